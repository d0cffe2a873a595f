"""Grain match: measure the grain of a photograph or video frame and put it back under the mask.

What the VAE decoder returns under the mask is clean; the image around it carries sensor noise, film grain or compression noise.
On a still the inpainted area reads as too smooth, on video as a patch of dirty glass that sits still while the grain around it
moves.  Colour match and seam blend cannot fix that.  Three steps and the noise itself, all on the device
(csrc/grain_kernel.hip; include/lanpaint_hip.h states the rule in full):

stats   grain_stats(image, mask, region, flat, margin) -> int64 [B, C, 8, 3]: per image, channel and tone band {n, sum e1^2,
        sum e2^2} of two noise operators (Immerkaer's 3 x 3 operator, and the same with its taps two pixels apart) on the image's
        8-bit codes, over the pixels whose 5 x 5 window lies inside the image, is flat (max - min <= `flat`) and lies in the
        region: "all", "outside" (every mask element within `margin` is <= 0.5) or "inside" (every mask element of the window is
        > 0.5).  Exact integers.

fit     grain_fit(gen, ref, strength, size, clip_frames) -> (amp fp32 [B, C, 8], size int32 [B]): what the reference side has
        and the generated side lacks, per channel and band, as the amplitude of a grain of size 0 (white), 1 (3 x 3 binomial) or
        2 (5 x 5 binomial); "auto" takes the size from the ratio of the two operators' energies.  Pooled per clip of
        `clip_frames` frames (0: the whole batch), fp64 with every operation rounded on its own.

field   grain_field(shape, size, seed, monochrome, frame0) -> int32 [B, H, W, C]: the integer grain, a function of (seed, frame,
        y, x, c, W, size) only -- Philox4x32-10 per lattice point -- so tiles and chunks cannot change it.

apply   grain_apply(image, mask, amp, size, ...) -> fp32 [B, H, W, C] = image + (mask * a) * g with a interpolated between tone
        bands; where mask * a is 0 the output is the input's bits.

match() calls them in turn.  HIP tensors only, no CPU fallback; the tables stay on the device and nothing is read back.  Frames
are measured and grained in chunks whose fp32 staging copies stay under WS_CAP_BYTES, with the frame number carried, so chunking
cannot change a bit.
"""
from __future__ import annotations

import ctypes

import torch

from . import _cabi
from ._hostcall import MAX_BATCH, chunks, float_in, image4, int_in, launch, mask_for, require_hip
from ._util import _as_f32c

BANDS = _cabi.LP_GRAIN_BANDS
MAX_MARGIN = _cabi.LP_GRAIN_MAX_MARGIN
MAX_FRAME0 = _cabi.LP_GRAIN_MAX_FRAME0
REGIONS = {"all": _cabi.LP_GRAIN_REGION_ALL, "outside": _cabi.LP_GRAIN_REGION_OUTSIDE, "inside": _cabi.LP_GRAIN_REGION_INSIDE}
SIZES = {"auto": _cabi.LP_GRAIN_SIZE_AUTO, "fine": 0, "medium": 1, "coarse": 2}
WS_CAP_BYTES = 1 << 30


def _size(size):
    """`size` as the C entry takes it: "auto" / "fine" / "medium" / "coarse", or -1..2."""
    if isinstance(size, str):
        if size not in SIZES:
            raise ValueError(f"size must be one of {tuple(SIZES)} or an integer in -1..2, got {size!r}")
        return SIZES[size]
    return int_in(size, -1, 2, "size")


def _check_stats(region, flat, margin):
    if region not in REGIONS:
        raise ValueError(f"region must be one of {tuple(REGIONS)}, got {region!r}")
    int_in(flat, 0, 255, "flat")
    int_in(margin, 0, MAX_MARGIN, "margin")


def _check_fit(batch, strength, size, clip_frames):
    float_in(strength, 0.0, 2.0, "strength")
    if int_in(clip_frames, 0, batch, "clip_frames") and batch % clip_frames:
        raise ValueError(f"clip_frames must be 0 or a divisor of the batch {batch}, got {clip_frames!r}")
    return _size(size)


def _check_field(seed, frame0):
    int_in(seed, 0, (1 << 64) - 1, "seed")
    int_in(frame0, 0, MAX_FRAME0, "frame0")


def _frames(img):
    """(start, count) over the frames of `img` [B, H, W, C]: a chunk's fp32 copy stays under WS_CAP_BYTES."""
    b, h, w, c = img.shape
    return chunks(b, h * w * c * 4, WS_CAP_BYTES)


def grain_stats(image, mask=None, region="all", flat=64, margin=8):
    """The noise statistics of `image` [B, H, W, C] as int64 [B, C, 8, 3] on the device (module docstring).  `mask` is
    [B, H, W], [1, H, W] or [H, W]; region "all" takes none."""
    _check_stats(region, flat, margin)
    img = image4(require_hip(image, "image", __name__), "image", MAX_BATCH)
    b, h, w, c = img.shape
    dev = img.device
    m = None
    if region != "all":
        if mask is None:
            raise ValueError(f"region {region!r} needs a mask")
        m = mask_for(require_hip(mask, "mask", __name__), b, h, w, dev)
    stats = torch.empty((b, c, BANDS, 3), dtype=torch.int64, device=dev)
    for s, n in _frames(img):
        part = _as_f32c(img[s:s + n])
        mp = None if m is None else m if m.shape[0] == 1 else m[s:s + n]
        d = _cabi.LpGrainStatsDesc(n, h, w, c, 1 if mp is None else mp.shape[0], margin, flat, REGIONS[region], part.data_ptr(),
                                   None if mp is None else mp.data_ptr(), stats[s:s + n].data_ptr())
        launch("lp_grain_stats", dev, ctypes.byref(d))
    return stats


def _table(t, what):
    if t.ndim != 4 or t.dtype != torch.int64 or t.shape[0] < 1 or tuple(t.shape[2:]) != (BANDS, 3) \
            or not 1 <= t.shape[1] <= _cabi.LP_DETAIL_MAX_CHANNELS or t.shape[0] > MAX_BATCH:
        raise ValueError(f"{what} must be int64 [B, C, {BANDS}, 3] with C in 1..{_cabi.LP_DETAIL_MAX_CHANNELS} and B in "
                         f"1..{MAX_BATCH}, got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def grain_fit(gen, ref, strength=1.0, size="auto", clip_frames=0):
    """grain_stats' tables of the generated side [B, C, 8, 3] and the reference side [Br, C, 8, 3] -> (amp fp32 [B, C, 8], size
    int32 [B]) on the device, by the rule of the module docstring.  One launch."""
    g = _table(require_hip(gen, "gen", __name__), "gen")
    r = _table(require_hip(ref, "ref", __name__).to(g.device), "ref")
    if r.shape[1] != g.shape[1]:
        raise ValueError(f"ref has {r.shape[1]} channels, gen {g.shape[1]}")
    b, c = g.shape[:2]
    s = _check_fit(b, strength, size, clip_frames)
    dev = g.device
    amp = torch.empty((b, c, BANDS), dtype=torch.float32, device=dev)
    size_out = torch.empty((b,), dtype=torch.int32, device=dev)
    d = _cabi.LpGrainFitDesc(b, r.shape[0], c, clip_frames, s, 0, float(strength), g.data_ptr(), r.data_ptr(), amp.data_ptr(),
                             size_out.data_ptr())
    launch("lp_grain_fit", dev, ctypes.byref(d))
    return amp, size_out


def grain_field(shape, size, seed=0, monochrome=False, frame0=0, device=None):
    """The integer grain of size 0..2 for `shape` = (B, H, W, C): int32 on the current (or the given) HIP device."""
    b, h, w, c = (int(v) for v in shape)
    int_in(size, 0, 2, "size")
    _check_field(seed, frame0)
    image4(torch.empty((b, h, w, c), device="meta"), "shape")
    if not torch.cuda.is_available():
        raise RuntimeError(f"{__name__} runs on a HIP device only; no CPU fallback")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    out = torch.empty((b, h, w, c), dtype=torch.int32, device=dev)
    for s, n in chunks(b, 1, MAX_BATCH):
        d = _cabi.LpGrainFieldDesc(n, h, w, c, size, int(bool(monochrome)), frame0 + s, seed, out[s:s + n].data_ptr())
        launch("lp_grain_field", dev, ctypes.byref(d))
    return out


def grain_apply(image, mask, amp, size, seed=0, monochrome=False, frame0=0):
    """`image` [B, H, W, C] with the grain of grain_fit's (amp, size) added under `mask` (module docstring): fp32, a new tensor.
    One launch per chunk of frames."""
    _check_field(seed, frame0)
    img = image4(require_hip(image, "image", __name__), "image", MAX_BATCH)
    b, h, w, c = img.shape
    dev = img.device
    m = mask_for(require_hip(mask, "mask", __name__), b, h, w, dev)
    a, sz = require_hip(amp, "amp", __name__), require_hip(size, "size", __name__)
    if tuple(a.shape) != (b, c, BANDS) or a.dtype != torch.float32:
        raise ValueError(f"amp must be float32 {(b, c, BANDS)}, got {a.dtype} {tuple(a.shape)}")
    if tuple(sz.shape) != (b,) or sz.dtype != torch.int32:
        raise ValueError(f"size must be int32 {(b,)}, got {sz.dtype} {tuple(sz.shape)}")
    a, sz = a.to(dev).contiguous(), sz.to(dev).contiguous()
    out = torch.empty((b, h, w, c), dtype=torch.float32, device=dev)
    for s, n in _frames(img):
        part = _as_f32c(img[s:s + n])
        mp = m if m.shape[0] == 1 else m[s:s + n]
        d = _cabi.LpGrainApplyDesc(n, h, w, c, mp.shape[0], int(bool(monochrome)), frame0 + s, seed, part.data_ptr(),
                                   mp.data_ptr(), a[s:s + n].data_ptr(), sz[s:s + n].data_ptr(), out[s:s + n].data_ptr())
        launch("lp_grain_apply", dev, ctypes.byref(d))
    return out


def match(image, mask, reference=None, strength=1.0, size="auto", monochrome=False, flat=64, margin=8, seed=0, clip_frames=0,
          frame0=0):
    """`image` [B, H, W, C] with the grain it lacks under `mask` put back.  The reference side is `reference` measured everywhere
    when given (any batch and size, the same channel count: a grain plate or the untouched original), otherwise `image`
    outside the mask; the generated side is `image` inside the mask.  On the current stream: two measurements (lp_grain_stats)
    and one apply per chunk of frames, and between them one fit for the whole batch; no device -> host read."""
    _check_stats("all", flat, margin)
    _check_fit(0, strength, size, 0)
    int_in(clip_frames, 0, MAX_BATCH, "clip_frames")
    _check_field(seed, frame0)
    img = image4(require_hip(image, "image", __name__), "image", MAX_BATCH)
    _check_fit(img.shape[0], strength, size, clip_frames)
    if reference is not None:
        ref_img = image4(require_hip(reference, "reference", __name__), "reference", MAX_BATCH)
        if ref_img.shape[3] != img.shape[3]:
            raise ValueError(f"reference has {ref_img.shape[3]} channels, image {img.shape[3]}")
        ref = grain_stats(ref_img.to(img.device), None, "all", flat)
    else:
        ref = grain_stats(img, mask, "outside", flat, margin)
    gen = grain_stats(img, mask, "inside", flat)
    amp, sz = grain_fit(gen, ref, strength, size, clip_frames)
    return grain_apply(img, mask, amp, sz, seed, monochrome, frame0)
