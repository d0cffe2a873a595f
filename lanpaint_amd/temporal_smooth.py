"""Video temporal smooth: what the sampler put under the mask stops boiling from frame to frame.

The sampler invents the content under the mask frame by frame; every step behind it treats a frame on its own.  Texture that
should be one piece of background therefore changes from frame to frame.  This follows the motion from every masked pixel a few
frames into the past and the future, looks at what the sampler put at the same scene point there, and pulls the pixel towards
the weighted mean of what agrees with it:

    decode / stitch -> temporal_smooth -> multiband blend -> grain match

Grain is synthesized afterwards, which is why smoothing it away here is wanted.

temporal_smooth(images, mask, radius=2, tolerance=24, motion="background", levels=4, search=2, smooth=8) -> (out, support)
        `images` [F, H, W, C]; `mask` [F, H, W], [1, H, W] or [H, W] (then the one mask serves every frame), binarised at 0.5.
        The motion from every frame to its two neighbours is the block field of `temporal_fill` (`levels`, `search`, `smooth`
        as there): with `motion="background"` weighted by the known pixels -- exactly the temporal fill's fields --, with
        `motion="picture"` by every pixel, for an inpainted subject that moves on its own.  A masked pixel's position is stepped
        along it, at most `radius` frames each way, and the picture is sampled there; a sample counts while no channel is more
        than `tolerance` grey levels (of 255) away from the pixel itself, and a chain ends at the first that does not.  The
        pixel moves to the binomially weighted mean of itself and what counted.  `out` fp32 [F, H, W, C]; `support` int32
        [F, H, W]: the samples that counted, 0..2 radius, and -1 outside the mask.  One frame or an empty mask returns the
        images; a clip whose masked area does not change along the field is returned bit for bit; nothing outside the mask
        changes; what is more than `tolerance` away is never averaged in.  include/lanpaint_hip.h (lp_tsmooth) states the rule
        in full.  Not done: a reference value other than the frame's own pixel, so a single outlier frame keeps its value,
        because every neighbour is rejected; motion boundaries finer than a block; a soft mask edge (the multiband blend
        follows).  `temporal_smooth_robust` is the robust form: a temporal median as the reference repairs an outlier frame.

HIP tensors only, no CPU fallback, no device -> host read.  The fields are independent jobs of lp_prop_match_batch /
lp_prop_fill_batch as in `temporal_fill`; the gather is one launch for all frames of a chunk (`smooth_frames`).  Pyramids and
fields are built for as many frames at a time as stay under WS_CAP_BYTES: a chunk of frames [lo, hi) needs the pyramids of the
frames lo - radius .. hi + radius - 1 clipped to the clip.  Nothing is carried from chunk to chunk, so chunking cannot change a
bit.  The fp32 copy of the clip that is sampled and the two outputs are held whole.
"""
from __future__ import annotations

import ctypes

import torch

from . import _cabi
from ._hostcall import chunks, int_in, launch, require_hip, tensor_is
from ._motion import check_images, check_params, clip_mask, luma_pyramids
from ._util import _as_f32c
from .temporal_fill import MAX_FRAMES, known_pyramids, step_fields

MAX_RADIUS = _cabi.LP_TSMOOTH_MAX_RADIUS
MOTIONS = ("background", "picture")
WS_CAP_BYTES = 1 << 30


def _numbers(radius, tolerance, motion):
    int_in(radius, 1, MAX_RADIUS, "radius")
    int_in(tolerance, 0, 255, "tolerance")
    if motion not in MOTIONS:
        raise ValueError(f"motion must be one of {MOTIONS}, got {motion!r}")


def field_steps(lo, hi, frames, radius):
    """What the walks of the frames lo .. hi - 1 of a clip of `frames` read: (the frames whose field towards the next frame, the
    frames whose field towards the one before), two ranges."""
    return range(lo, min(hi + radius - 1, frames - 1)), range(max(lo - radius + 1, 1), hi)


def launch_frames(entry, desc, planes, fwd, bwd, known, images, radius, tolerance, first, count, fwd_first, bwd_first):
    """What `smooth_frames` and `temporal_smooth_robust.robust_frames` share: the checks, and the call of `entry` with the
    descriptor `desc`.  `planes`: the outputs behind `out`, int32 [F, H, W] each, as (given or None, name).  Returns the outputs."""
    int_in(radius, 1, MAX_RADIUS, "radius")
    int_in(tolerance, 0, 255, "tolerance")
    F, H, W, C = check_images(images).shape
    int_in(F, 1, MAX_FRAMES, "the frame count")
    int_in(first, 0, F - 1, "first")
    count = int_in(F - first if count is None else count, 1, F - first, "count")
    dev = images.device
    (out, _), planes = planes[0], planes[1:]
    out = torch.empty((F, H, W, C), dtype=torch.float32, device=dev) if out is None else out
    planes = [(torch.empty((F, H, W), dtype=torch.int32, device=dev) if t is None else t, what) for t, what in planes]
    grid = _cabi.prop_grid(H, W)
    need = field_steps(first, first + count, F, radius)
    rows = []
    for t, start, steps, what in ((fwd, fwd_first, need[0], "fwd"), (bwd, bwd_first, need[1], "bwd")):
        if t is None:
            if len(steps):
                raise ValueError(f"{what} is needed for the frames {steps[0]}..{steps[-1]}")
            rows.append((None, 0, 0))
            continue
        tensor_is(t, torch.int32, (None, *grid, 2), what, __name__)
        int_in(start, 0, F - 1, f"{what}_first")
        if len(steps) and (start > steps[0] or start + t.shape[0] <= steps[-1]):
            raise ValueError(f"{what} holds the frames {start}..{start + t.shape[0] - 1}, the walks read {steps[0]}..{steps[-1]}")
        rows.append((t.data_ptr() if t.shape[0] else None, start, t.shape[0]))
    require_hip(known, "known", __name__)
    if known.dtype != torch.uint8 or known.ndim not in (2, 3) or known.shape[0] != count or known[0].numel() < H * W \
            or (known.ndim == 3 and tuple(known.shape[1:]) != (H, W)) or not known.is_contiguous():
        raise ValueError(f"known must be a contiguous uint8 [{count}, {H}, {W}] or frame pyramids [{count}, stride], got "
                         f"{known.dtype} {list(known.shape)}")
    for t, dtype, shape, what in ((images, torch.float32, (F, H, W, C), "images"), (out, torch.float32, (F, H, W, C), "out"),
                                  *((t, torch.int32, (F, H, W), what) for t, what in planes)):
        tensor_is(t, dtype, shape, what, __name__)
    (f_ptr, f_first, f_n), (b_ptr, b_first, b_n) = rows
    d = desc(F, H, W, C, first, count, radius, tolerance, f_first, f_n, b_first, b_n, f_ptr, b_ptr, known.data_ptr(), known[0].numel(),
             images.data_ptr(), out.data_ptr(), *(t.data_ptr() for t, _ in planes))
    launch(entry, dev, ctypes.byref(d))
    return (out, *(t for t, _ in planes))


def smooth_frames(fwd, bwd, known, images, radius=2, tolerance=24, first=0, count=None, fwd_first=0, bwd_first=1, out=None,
                  support=None):
    """The one launch: the frames first .. first + count - 1 (to the clip's end by default) of `images` fp32 [F, H, W, C] are
    smoothed into `out` and `support` (new when not given: the other frames are then left unwritten).  `fwd` int32
    [n, gh, gw, 2]: row j is the level-0 final field of frame fwd_first + j towards the next frame; `bwd` likewise of frame
    bwd_first + j towards the one before; they must cover `field_steps(first, first + count, F, radius)` and may be None where
    that is empty.  `known` uint8 [count, H, W], or frame pyramids [count, stride]: the bits of the frames written.
    Returns (out, support)."""
    return launch_frames("lp_tsmooth", _cabi.LpTsmoothDesc, ((out, "out"), (support, "support")), fwd, bwd, known, images, radius,
                          tolerance, first, count, fwd_first, bwd_first)


def over_chunks(frames_fn, planes, images, mask, radius, tolerance, motion, levels, search, smooth):
    """The whole call of `temporal_smooth` and of `temporal_smooth_robust.temporal_smooth_robust`: the fields chunk by chunk, and
    `frames_fn` (`smooth_frames` or `robust_frames`) on every chunk, into `out` and `planes` int32 [F, H, W] held whole."""
    _numbers(radius, tolerance, motion)
    check_params(levels, search, smooth)
    check_images(images)
    F, H, W, C = images.shape
    int_in(F, 1, MAX_FRAMES, "the frame count")
    dev = images.device
    mask = _as_f32c(clip_mask(mask, F, H, W, __name__).to(dev))
    images = _as_f32c(images)                                            # what is sampled; `out` is written next to it
    out = torch.empty((F, H, W, C), dtype=torch.float32, device=dev)
    outputs = (out, *(torch.empty((F, H, W), dtype=torch.int32, device=dev) for _ in range(planes)))
    stride = _cabi.prop_pyramid_ws_bytes(1, H, W, levels)
    gh, gw = _cabi.prop_grid(H, W)
    per_frame = (3 if motion == "picture" else 2) * stride + 2 * gh * gw * 8     # a frame's pyramids and its two fields
    for lo, n in chunks(F, per_frame, max(WS_CAP_BYTES - 2 * radius * per_frame, 1)):
        hi = lo + n
        p_lo, p_hi = max(lo - radius, 0), min(hi + radius, F)            # the frames whose pyramids the fields need
        known = known_pyramids(mask if mask.shape[0] == 1 else mask[p_lo:p_hi], p_hi - p_lo, levels)
        fwd, bwd = field_steps(lo, hi, F, radius)
        steps = [(u - p_lo, u + 1 - p_lo) for u in fwd] + [(u - p_lo, u - 1 - p_lo) for u in bwd]
        fields = None
        if steps:
            luma = luma_pyramids(images[p_lo:p_hi], levels)
            weights = known if motion == "background" else known_pyramids(torch.zeros((1, H, W), dtype=torch.float32, device=dev),
                                                                          p_hi - p_lo, levels)
            fields = step_fields(luma, weights, steps, H, W, levels, search, smooth)
            del luma, weights
        frames_fn(fields[:len(fwd)] if len(fwd) else None, fields[len(fwd):] if len(bwd) else None, known[lo - p_lo:hi - p_lo],
                  images, radius, tolerance, lo, n, fwd[0] if len(fwd) else 0, bwd[0] if len(bwd) else 0, *outputs)
    return outputs


def temporal_smooth(images, mask, radius=2, tolerance=24, motion="background", levels=4, search=2, smooth=8):
    """What lies under `mask` in the frames `images` [F, H, W, C], pulled towards what the neighbouring frames hold at the same
    scene point (module docstring): (out fp32 [F, H, W, C], support int32 [F, H, W]) on the images' device.  No device -> host
    read."""
    return over_chunks(smooth_frames, 1, images, mask, radius, tolerance, motion, levels, search, smooth)
