"""The image-space family on the MI355X where its own suites do not look, as tests/test_gpu_motion_scratch.py does it for the motion
family: outputs, workspaces and tables that hold a poison before the call, a side stream that is held back while the call is made,
and the docstrings' device -> host reads and launches, counted.

The family is what _hostcall.py lists -- video mask, audio merge, blend, the four Detailer forms, colour match, fill, multiband,
refine, stabilize -- and grain match.  Every public call and the stage functions that allocate their own results run with every
`torch.empty` / `torch.empty_like` filled with 0x00 and with 0xFF (tests/poison.py): outputs, `detail._resample`'s scratch, the
label workspace and table, the EDT's int32 / fp64 / int64 planes, the colour match's fp64 workspace and table, the grain tables and
the byte workspaces all come from there.  A cell read before it is written, an output element nobody writes or an integer table
that is added to before it is reset shows as different bits; on the allocator's warm blocks it does not.  Each comparison is the
one the call's own suite applies to that call -- bit for bit wherever the suite is; elsewhere the suite's derived bound: the tap
table bound of the Detailer's resample and stitch, the fp64 summation bound of the colour sums, the audio merge's restatement --
and no tolerance is added.

0x00 and 0xFF (-1) and nothing wilder.  Read before the first run (CHANGES.md, round 42): no image-space kernel turns a value
loaded from such a buffer into an index, an offset or a loop bound without a range check or a clamp, and both values stay next to
the buffer should one ever be used raw.
"""
import functools
import time

import numpy as np
import pytest
import torch

from lanpaint_amd import (_cabi, _util, audio, blend, detail, detail_color, detail_subjects, fill, grain, multiband, refine,
                          resample, stabilize, videomask)
from oracle import lanpaint_oracle as orc
from tests import color_ref, compare, detail_ref, device, fill_ref, image_checks, image_inputs, regions_ref, subjects_ref
from tests import grain_ref as gref
from tests import multiband_ref as mb_ref
from tests import refine_ref as rref
from tests import stabilize_ref as sref
from tests import videomask_ref as vref
from tests.audio_ref import lerp_f32, weights_f64
from tests.compare import ulps
from tests.device import DEV, _dev, _spin_cycles_per_ms
from tests.helpers import record_launches
from tests.inputs import LARGE, SMALL
from tests.poison import POISONS, poison_id, poisoned_empty

pytestmark = pytest.mark.gpu
# (23, 33) and (40, 70): odd, no multiple of a tile side (16, 32, 64), of the 16 x 64 grain and label tiles, of the 1024-element
# label chunk or of the stabilize's 256-pixel block; (40, 70) takes several workgroups of every kernel and three label chunks.
# B = 3 images; a config is (plane, channels, mask planes): C = 3 has W * C % 4 != 0, the element-wise forms, C = 4 on (40, 70) the
# float4 forms; the mask is once one plane for all images and once a plane each.  "chunked": fp16 images (the restatement on the
# half-rounded values) and the module's WS_CAP_BYTES lowered until a chunk holds one image, or for stabilize one time segment.
B, FRAMES, CLIP = 3, 18, 5                                             # FRAMES: more than one LP_STAB_SEG_FRAMES; CLIP: the Detailer's video
CONFIGS = [(SMALL, 3, 1), (LARGE, 3, B), (LARGE, 4, 1)]
CHUNKED = [(SMALL, 3, B), (LARGE, 3, B)]
MODULES = (audio, blend, detail, detail_color, detail_subjects, fill, grain, multiband, refine, resample, stabilize, videomask)
K, K_WIDE, FILTER = 9, 17, "bicubic"                                   # blend_overlap: the 16 x 64 tile and, above 15, the 8 x 32 one


def _bits(a):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = _bits(got) != _bits(want)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def _half(a, mode):
    """`a` as the chunked mode hands it over: rounded to fp16 (the device gets the fp16 tensor, the restatement these values)."""
    return a.astype(np.float16).astype(np.float32) if mode == "chunked" else a


def _halves(mode, *indices):
    """The inputs, by index, that the chunked mode uploads as fp16."""
    return indices if mode == "chunked" else ()


def _gen(*key):
    return torch.Generator().manual_seed(int(np.random.default_rng(list(key)).integers(1 << 31)))


class Case:
    """One call at one shape.  `inputs`: numpy arrays (or None) that `device()` uploads, those at `halves` as fp16; `run(*dev)`
    makes the call and returns what it returns; `check(got, dev, what)` applies the suite's comparison (it may launch more work:
    the launches and reads of the call itself are taken before it runs); `caps(monkeypatch)` lowers the caps of the chunked mode;
    `launches(names, chunked)` holds the C entries the call launched to its docstring."""

    def __init__(self, inputs, run, check, halves=(), caps=None, launches=None, allocates=True):
        self.inputs, self.run, self.check, self.halves, self.caps, self.launches, self.allocates = \
            inputs, run, check, frozenset(halves), caps, launches, allocates

    def device(self):
        return tuple(None if a is None else _dev(a).half() if i in self.halves else _dev(a) for i, a in enumerate(self.inputs))


def _only(names, **counts):
    """`names` holds exactly `counts[entry]` launches of each entry and no other."""
    assert {e: names.count(e) for e in counts} == counts and len(names) == sum(counts.values()), (names, counts)


# ---- fill ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fill_masked(plane, C, Bm, mode):
    H, W = plane
    img, mask = image_inputs._image(B, H, W, C, 3), image_inputs._fill_speckle(Bm, H, W, 5)
    if Bm == B:
        mask[1] = 1.0                                                  # one image with no known pixel: it comes back unchanged
        assert not (~(mask[1] > 0.5)).any() and (~(mask[0] > 0.5)).any() and (mask[0] > 0.5).any()
    want = fill_ref.fill_ref(img, mask)
    levels = len(fill_ref.levels(H, W))

    def check(got, dev, what):
        got = got.cpu().numpy()
        assert got.dtype == np.float32 and got.shape == img.shape, what
        bad = got != want
        assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        known = np.broadcast_to(~(mask > 0.5), img.shape[:3])
        assert (_bits(got)[known] == _bits(img)[known]).all(), what
        if Bm == B:
            assert (_bits(got[1]) == _bits(img[1])).all(), what

    def launches(names, chunked):
        _only(names, lp_mask_fill=1)                                   # one entry: a pull and a push launch per span of five levels
        assert 2 * -(-(levels - 1) // _cabi.LP_FILL_SPAN) <= 6

    return Case((img, mask), fill.fill_masked, check, launches=launches)


@functools.lru_cache(maxsize=None)
def _outpaint_pad(plane, C, Bm, mode, do_fill, with_mask):
    H, W = plane
    img = image_inputs._image(B, H, W, C, 8)
    mask = image_inputs._fill_speckle(Bm, H, W, 25) * np.float32(0.8) if with_mask else None
    pads = dict(left=5, top=0, right=3, bottom=6, overlap=2, multiple_of=8)
    plan = fill.plan_outpaint(H, W, **pads)
    want_c, want_m = fill_ref.pad_ref(img, mask, plan.left, plan.top, plan.right, plan.bottom, plan.overlap)
    if do_fill:
        want_c = fill_ref.fill_ref(want_c, want_m)

    def check(got, dev, what):
        canvas, m = (t.cpu().numpy() for t in got)
        assert (_bits(m) == _bits(want_m)).all(), what
        if do_fill:
            assert canvas.shape == want_c.shape and (canvas == want_c).all(), what
        else:
            assert canvas.shape == want_c.shape and (_bits(canvas) == _bits(want_c)).all(), what

    def launches(names, chunked):
        _only(names, lp_outpaint_pad=1, lp_mask_fill=int(do_fill))

    return Case((img, mask), lambda i, m: fill.outpaint_pad(i, m, fill=do_fill, **pads), check, launches=launches)


# ---- multiband ------------------------------------------------------------------------------------------------------------------------------
LEVELS = 5


@functools.lru_cache(maxsize=None)
def _blend_multiband(plane, C, Bm, mode):
    H, W = plane
    a, b = _half(image_inputs._image(B, H, W, C, 11), mode), _half(image_inputs._image(B, H, W, C, 12), mode)
    mask = image_inputs._soft(Bm, H, W, 13)
    want = mb_ref.blend_ref(a, b, mask, LEVELS)

    def check(got, dev, what):
        got = got.cpu().numpy()
        assert got.dtype == np.float32 and got.shape == a.shape, what
        bad = got != want
        assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())

    def caps(monkeypatch):
        monkeypatch.setattr(multiband, "WS_CAP_BYTES", _cabi.multiband_ws_bytes(1, H, W, C, LEVELS) + 8)

    def launches(names, chunked):
        _only(names, lp_multiband_blend=B if chunked else 1)

    return Case((a, b, mask), lambda x, y, m: multiband.blend_multiband(x, y, m, LEVELS), check, _halves(mode, 0, 1), caps, launches)


# ---- refine ---------------------------------------------------------------------------------------------------------------------------------
def _refine_caps(plane):
    """One image a chunk of the filter and one frame a chunk of the EDT: both take 16 bytes a pixel."""
    H, W = plane
    assert _cabi.refine_ws_bytes(1, H, W, 3, 8) == videomask.EDT_BYTES_PER_PIXEL * H * W
    return lambda monkeypatch: monkeypatch.setattr(refine, "WS_CAP_BYTES", videomask.EDT_BYTES_PER_PIXEL * H * W + 8)


def _soft_blobs(Bm, H, W, mode):
    """tests/test_gpu_refine.py's blobs with soft values: above 0.5 inside, below it outside."""
    soft = image_inputs._soft(Bm, H, W, 7)
    m = np.where(image_inputs._refine_blobs(Bm, H, W) > 0, np.float32(0.5) + np.float32(0.5) * soft,
                 np.float32(0.499) * soft).astype(np.float32)
    return _half(m, mode)


@functools.lru_cache(maxsize=None)
def _grow_mask(plane, C, Bm, mode, grow):
    H, W = plane
    mask = _soft_blobs(Bm, H, W, mode)
    want = np.stack([rref.grow_ref(m, grow) for m in mask])
    assert want.any() and not want.all() and (want != (mask >= 0.5)).any()

    def check(got, dev, what):
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == mask.shape, what
        assert (got.cpu().numpy() == want).all(), what

    def launches(names, chunked):
        _only(names, lp_vmask_edt=Bm if chunked else 1)

    return Case((mask,), lambda m: refine.grow_mask(m, grow), check, _halves(mode, 0), _refine_caps(plane), launches)


@functools.lru_cache(maxsize=None)
def _refine_mask(plane, C, Bm, mode, radius, grow):
    H, W = plane
    guide, mask = _half(image_inputs._guide(B, H, W, C, 11), mode), image_inputs._soft(Bm, H, W, 13)
    grown = mask if grow == 0 else np.stack([rref.grow_ref(m, grow) for m in mask])
    want = rref.refine_ref(guide, grown, radius, 1e-3) if radius else np.ascontiguousarray(np.broadcast_to(grown, (B, H, W)))

    def check(got, dev, what):
        assert got.is_cuda and tuple(got.shape) == (B, H, W), what
        _same_bits(got, want, what)

    def launches(names, chunked):
        # per chunk of images the filter's one entry (its two launches, coeff and apply), besides the EDT's per chunk of mask
        # planes; radius 0 launches no filter, grow 0 no EDT, both 0 nothing at all
        _only(names, lp_mask_refine=(B if chunked else 1) if radius else 0, lp_vmask_edt=(Bm if chunked else 1) if grow else 0)

    return Case((guide, mask), lambda g, m: refine.refine_mask(g, m, radius=radius, eps=1e-3, grow=grow), check, _halves(mode, 0),
                _refine_caps(plane), launches, allocates=bool(radius or grow))


# ---- stabilize ------------------------------------------------------------------------------------------------------------------------------
STAB = (1, 2, 0.5, 3.0)                                                # median, smooth, grow, feather


@functools.lru_cache(maxsize=None)
def _stabilize_masks(plane, C, Bm, mode):
    H, W = plane
    mask = image_inputs._stabilize_blobs(FRAMES, H, W, 15)
    mask[1] = image_inputs._stabilize_soft(1, H, W, 3)[0]                              # a soft frame: the half rounding moves values across 0.5
    mask = _half(mask, mode)
    want = sref.stabilize_ref(mask, *STAB)
    assert FRAMES > _cabi.LP_STAB_SEG_FRAMES and not mask[FRAMES // 3].any()

    def check(got, dev, what):
        _same_bits(got, want, what)

    def caps(monkeypatch):                                             # one segment of frames a chunk of the EDT
        monkeypatch.setattr(stabilize, "WS_CAP_BYTES", _cabi.LP_STAB_SEG_FRAMES * videomask.EDT_BYTES_PER_PIXEL * H * W + 8)

    def launches(names, chunked):
        chunks = -(-FRAMES // _cabi.LP_STAB_SEG_FRAMES) if chunked else 1
        _only(names, lp_vmask_edt=chunks, lp_mask_signed_d2=chunks, lp_mask_stabilize=1)

    return Case((mask,), lambda m: stabilize.stabilize_masks(m, *STAB), check, _halves(mode, 0), caps, launches)


# ---- grain ----------------------------------------------------------------------------------------------------------------------------------
GRAIN = dict(margin=2, seed=3, frame0=5)                               # margin 2: the small plane keeps pixels outside the mask


def _grain_scene(plane, C, Bm, mode):
    """tests/test_gpu_grain.py's video: a noisy image that is clean under a box mask."""
    H, W = plane
    mask = image_inputs._box(B, H, W, Bm == B)
    clean = np.linspace(0.2, 0.8, W, dtype=np.float32)[None, None, :, None]
    image = np.where(mask[..., None] > 0.5, clean, image_inputs.IMAGES["medium"](B, H, W, C)).astype(np.float32)
    return _half(image, mode), mask


@functools.lru_cache(maxsize=None)
def _grain_match(plane, C, Bm, mode, with_plate, clip):
    H, W = plane
    image, mask = _grain_scene(plane, C, Bm, mode)
    plate = _half(image_inputs.IMAGES["coarse"](2, H + 3, W - 2, C, 9), mode) if with_plate else None
    want = gref.match(image, mask, plate, clip_frames=clip, **GRAIN)
    # the poison has to matter: pixels are measured outside the mask, and a band that no pixel touches holds the memset's zero
    outside = gref.grain_stats(image, mask, grain.REGIONS["outside"], 64, GRAIN["margin"])[..., 0]
    assert outside.sum() > 0 and (outside == 0).any() and (want != image).any()

    def check(got, dev, what):
        compare._same_typed(got.cpu().numpy(), want, what)

    def caps(monkeypatch):                                             # one frame a chunk, of the image and of the larger plate
        monkeypatch.setattr(grain, "WS_CAP_BYTES", H * W * C * 4 + 8)

    def launches(names, chunked):
        chunks = B if chunked else 1
        measured = chunks + ((2 if chunked else 1) if with_plate else chunks)
        _only(names, lp_grain_stats=measured, lp_grain_fit=1, lp_grain_apply=chunks)
        assert with_plate or measured == 2 * chunks                    # two measurements and one apply per chunk, one fit

    return Case((image, mask, plate), lambda i, m, p: grain.match(i, m, p, clip_frames=clip, **GRAIN), check, _halves(mode, 0, 2), caps,
                launches)


# ---- colour match -----------------------------------------------------------------------------------------------------------------------------
MARGIN, SMOOTH = 2, 3


@functools.lru_cache(maxsize=None)
def _color_match(plane, C, Bm, mode, method):
    H, W = plane
    (d, r), mask = image_inputs._images(B, H, W, C, 1), image_inputs._blob_mask(Bm, H, W, 2)
    want_stats, mag = color_ref.stats_ref(d, r, mask, MARGIN)
    assert (want_stats[:, 0] >= _cabi.LP_COLOR_MIN_COUNT).all() and (want_stats[:, 0] < H * W).all()

    def check(got, dev, what):
        """The stages' comparisons, composed: the sums inside their fp64 bound (n exactly), then the fit from the device's own
        sums and the apply of that fit, both bit for bit; the sums' bits are the same on every call."""
        stats = detail_color.color_stats(*dev, MARGIN).cpu().numpy()
        assert (stats[:, 0] == want_stats[:, 0]).all(), (what, stats[:, 0], want_stats[:, 0])
        bound = want_stats[:, :1] * 2.0 ** -52 * mag[:, 1:]
        err = np.abs(stats[:, 1:] - want_stats[:, 1:])
        assert (err <= bound).all(), (what, float((err / np.maximum(bound, 1e-300)).max()))
        coef = color_ref.fit_ref(stats, method, 1.0, SMOOTH, 0)
        assert (coef != np.float32([1.0, 0.0])).any()
        _same_bits(got, color_ref.apply_ref(d, coef), what)

    def launches(names, chunked):                                      # four launches: the sums are a tile launch and a fold
        assert names == ["lp_color_stats", "lp_color_fit", "lp_color_apply"], names

    return Case((d, r, mask), lambda x, y, m: detail_color.match(x, y, m, method, 1.0, MARGIN, SMOOTH, 0), check, launches=launches)


# ---- blend and audio --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mask_blend(plane, C, Bm, mode):
    H, W = plane
    i1, i2, mask = image_inputs._image(B, H, W, C, 1), image_inputs._image(B, H, W, C, 2), image_inputs._multiband_speckle(Bm, H, W, 4)
    want = orc.mask_blend(i1, i2, np.ascontiguousarray(np.broadcast_to(mask, (B, H, W))), K)

    def check(got, dev, what):
        np.testing.assert_allclose(got.cpu().numpy(), want, atol=3e-6, err_msg=str(what))

    return Case((i1, i2, mask), lambda a, b, m: blend.mask_blend(a, b, m, K), check,
                launches=lambda names, chunked: _only(names, lp_mask_blend=1))


@functools.lru_cache(maxsize=None)
def _merge_video(plane, C, Bm, mode, half_res):
    H, W = plane
    o, p = image_inputs._image(B, H, W, C, 3), image_inputs._image(B, H, W, C, 4)
    mask = image_inputs._multiband_speckle(Bm, H // 2, W // 2, 5) if half_res else image_inputs._multiband_speckle(Bm, H, W, 6)
    want = orc.merge_video_with_mask(o, p, mask, K_WIDE, mask_on="gpu")   # the mask is on the device: torch's GPU index rule

    def check(got, dev, what):
        np.testing.assert_allclose(got.cpu().numpy(), want, atol=3e-6, err_msg=str(what))

    return Case((o, p, mask), lambda a, b, m: blend.merge_video_with_mask(a, b, m, K_WIDE), check,
                launches=lambda names, chunked: _only(names, lp_mask_blend=1))


SR, CROSSFADE, MASK_FRAMES = 1000, 0.011, 7                            # cf = 11 samples: the prefix workspace exists


@functools.lru_cache(maxsize=None)
def _merge_audio(n):
    rng = np.random.default_rng([n, 5])
    orig, inp = (np.float32(0.3) * rng.standard_normal((1, 2, n)).astype(np.float32) for _ in range(2))
    am = rng.random(MASK_FRAMES, dtype=np.float32)
    cf = audio.crossfade_samples(CROSSFADE, SR)
    assert cf > 1
    want_w = weights_f64(am, n, cf, _cabi.LP_NN_ATEN_SCALAR)

    def merge(o, p, m):
        return audio.merge_audio_with_mask(o, p, m, CROSSFADE, SR, SR)

    def check(got, dev, what):
        """tests/test_gpu_av_merge.py's restatement comparison: w' as the kernel computes it -- the merge of zeros into ones --
        within 2 ulps of the float64 restatement, and the blend exact fp32 arithmetic on the kernel's own w'."""
        w = merge(torch.zeros(1, 1, n, device=DEV), torch.ones(1, 1, n, device=DEV), dev[2])[0, 0].cpu().numpy()
        assert ulps(w, want_w).max() <= 2, what
        assert got.is_cuda and got.dtype == torch.float32
        np.testing.assert_array_equal(got.cpu().numpy(), lerp_f32(orig, inp, w[None, None]), err_msg=str(what))

    return Case((orig, inp, am), merge, check, launches=lambda names, chunked: _only(names, lp_audio_merge=1))


# ---- video mask -------------------------------------------------------------------------------------------------------------------------------
INDICES, COUNT = (2, 7, 11, 12), 15


@functools.lru_cache(maxsize=None)
def _interpolate_masks(plane, C, Bm, mode):
    """tests/test_gpu_videomask_shapes.py's end-to-end case on this plane, with a resize up on both axes."""
    h, w = plane
    rng = np.random.default_rng(h + w)
    keys = np.stack([image_inputs._blob(rng, h, w) for _ in INDICES])
    size = (w + 17, h + 9)
    centroids = []
    for k in keys:
        ys, xs = np.nonzero(k >= 0.5)
        centroids.append((int(ys.sum()) / len(ys), int(xs.sum()) / len(xs)) if len(ys) else None)
    assert all(c is not None for c in centroids)
    want = vref.pil_resize_ref(vref.codes_ref(vref.morph_ref(keys, videomask.frame_plan(list(INDICES), COUNT, centroids))), size)

    def check(got, dev, what):
        got = got.cpu().numpy()
        assert got.shape == want.shape and got.dtype == np.float32, what
        assert np.abs(got - want).max() <= 1.0 / 255.0 + 1e-7, what
        assert np.mean(got == want) >= 0.9999, what
        assert not got[:2].any() and not got[13:].any() and got[3:7].any(), what

    def run(stack):
        return videomask.interpolate_masks({i: stack[j] for j, i in enumerate(INDICES)}, COUNT, size=size, device=DEV)

    return Case((keys,), run, check, launches=lambda names, chunked: _only(names, lp_vmask_edt=1, lp_vmask_morph=1, lp_vmask_resize=1))


# ---- the Detailer -------------------------------------------------------------------------------------------------------------------------------
# Two blobs as fractions of the plane, rows and columns apart, soft above 0.5 inside and soft at or below 0.3 outside (nobody's).
BLOBS = ((0.09, 0.34, 0.09, 0.33), (0.57, 0.90, 0.58, 0.90))            # (y0, y1, x0, x1), exclusive ends
TARGET = 24                                                            # every window is resampled: scratch and tables exist


def _soften(S, seed):
    noise = torch.rand(S.shape, generator=_gen(*S.shape, seed))
    return torch.where(S, 0.55 + 0.45 * noise, 0.3 * noise * (noise > 0.8))


def _two_blobs(Bm, H, W):
    """Blob i on plane i % Bm: with one plane both are on it, with B planes each is on its own and plane 2 is empty."""
    S = torch.zeros(Bm, H, W, dtype=torch.bool)
    for i, (y0, y1, x0, x1) in enumerate(BLOBS):
        S[i % Bm, int(y0 * H):int(y1 * H), int(x0 * W):int(x1 * W)] = True
    return _soften(S, 1)


def _two_subjects(H, W, empty=None):
    """CLIP frames: the upper blob moves right two steps a frame and the lower one left one step, each less than its width, so
    that a blob is one component in space and time and their common box moves; frame `empty` holds nothing."""
    S = torch.zeros(CLIP, H, W, dtype=torch.bool)
    step = max(1, W // 30)
    for f in range(CLIP):
        if f == empty:
            continue
        for i, (y0, y1, x0, x1) in enumerate(BLOBS):
            dx = 2 * f * step if i == 0 else -f * step
            assert 0 <= int(x0 * W) + dx and int(x1 * W) + dx <= W
            S[f, int(y0 * H):int(y1 * H), int(x0 * W) + dx:int(x1 * W) + dx] = True
    return _soften(S, 2)


def _resample_check(got, src, region, filter, what):
    """tests/test_gpu_detail.py's: the window of `src` [B, H, W, C] (CPU) through torch's fp64 operator, inside the tap-table bound."""
    r = region
    crop = src[:, r.y0:r.y0 + r.h, r.x0:r.x0 + r.w, :].contiguous()
    want = detail_ref.ref64(crop, (r.oh, r.ow), filter)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape), what
    e = float((got.cpu().double() - want).abs().max())
    assert e <= detail_ref.bound((r.h, r.w), (r.oh, r.ow), filter, float(crop.abs().max())), (what, e)


def _stitch_bound(win, filter, det):
    return 3e-6 + detail_ref.bound((win.oh, win.ow), (win.h, win.w), filter, float(det.abs().max()))


@functools.lru_cache(maxsize=None)
def _single_scene(plane, C, Bm):
    H, W = plane
    image, mask = torch.rand(B, H, W, C, generator=_gen(H, W, C, 1)), _two_blobs(Bm, H, W)
    bbox = image_checks._bbox_ref(mask)
    region = detail.plan_region(bbox, H, W, 1.0, 1, 8, 2 * TARGET)
    assert region.resampled and (region.h, region.w) != (H, W)
    det = torch.rand(B, region.oh, region.ow, C, generator=_gen(H, W, C, 2))
    return image, mask, bbox, region, det


def _single_stitch_check(got, original, det, mask, region, what):
    out = got.cpu()
    err = float((out - detail_ref.stitch_ref(original, det, mask, region, K, FILTER)).abs().max())
    assert err <= _stitch_bound(region, FILTER, det), (what, err)
    assert image_checks._outside_is_untouched(out, original, region), what


@functools.lru_cache(maxsize=None)
def _detail_single(plane, C, Bm, mode, call):
    image, mask, bbox, region, det = _single_scene(plane, C, Bm)
    if call == "mask_bbox":
        def check(got, dev, what):
            assert got == bbox, (what, got, bbox)
        return Case((mask.numpy(),), detail.mask_bbox, check, launches=lambda names, chunked: _only(names, lp_mask_bbox=1))
    if call == "crop_resample":
        def check(got, dev, what):
            _resample_check(got[0], image, region, FILTER, (what, "image"))
            _resample_check(got[1].unsqueeze(-1), mask.unsqueeze(-1), region, "bilinear", (what, "mask"))
            assert tuple(got[1].shape) == (Bm, region.oh, region.ow)
        return Case((image.numpy(), mask.numpy()), lambda i, m: detail.crop_resample(i, m, region, FILTER), check,
                    launches=lambda names, chunked: _only(names, lp_detail_resample=2))
    assert call == "stitch"
    return Case((image.numpy(), det.numpy(), mask.numpy()), lambda o, d, m: detail.stitch(o, d, m, region, K, FILTER),
                lambda got, dev, what: _single_stitch_check(got, image, det, mask, region, what),
                launches=lambda names, chunked: _only(names, lp_detail_resample=1, lp_detail_stitch=1))


@functools.lru_cache(maxsize=None)
def _regions_scene(plane, C, Bm):
    H, W = plane
    image, mask = torch.rand(B, H, W, C, generator=_gen(H, W, C, 3)), _two_blobs(Bm, H, W)
    labels, n, table = regions_ref.components_of(regions_ref.union_set(mask.numpy()))
    # fewer components than the table holds: the rows up to n are all compared, those beyond it never are
    assert n == len(BLOBS) < _cabi.LP_DETAIL_MAX_COMPONENTS
    regions = detail.plan_regions((n, table), H, W, 1.0, 1, 2, TARGET)
    assert len(regions) == n and regions.resampled and regions.members == ((1,), (2,))
    masks = [regions_ref.region_mask(mask, labels, mem) for mem in regions.members]
    assert sum(int((m != mask).sum()) for m in masks) > 0              # a region's view erases the other's component
    det = torch.rand(n * B, regions.oh, regions.ow, C, generator=_gen(H, W, C, 4))
    return image, mask, labels, n, table, regions, masks, det


def _regions_stitch_check(got, dev_original, dev_det, original, det, mask, labels, regions, masks, what):
    """tests/test_gpu_detail_regions.py's: the composition of `stitch` in region order bit for bit, and the torch restatement."""
    out = dev_original
    for i in range(len(regions)):
        out = detail.stitch(out, dev_det[i * B:(i + 1) * B], masks[i].to(DEV), regions.region(i), K, "bilinear")
    assert np.array_equal(_bits(got), _bits(out)), what
    cover = int(regions_ref.cover_count(regions).max())
    err = float((got.cpu() - regions_ref.stitch_regions_ref(original, det, mask, regions, labels, K, "bilinear")).abs().max())
    assert err <= cover * _stitch_bound(regions, "bilinear", det), (what, err)


@functools.lru_cache(maxsize=None)
def _detail_regions(plane, C, Bm, mode, call):
    image, mask, labels, n, table, regions, masks, det = _regions_scene(plane, C, Bm)
    if call == "mask_components":
        def check(got, dev, what):
            got_labels, got_n, got_table = got
            assert got_labels.is_cuda and got_labels.dtype == torch.int32 and got_n == n, (what, got_n)
            assert np.array_equal(got_labels.cpu().numpy(), labels) and got_table == table, what
        return Case((mask.numpy(),), detail.mask_components, check, launches=lambda names, chunked: _only(names, lp_mask_components=1))
    if call == "crop_regions":
        def check(got, dev, what):
            cimg, cmask = got
            assert tuple(cimg.shape) == (n * B, regions.oh, regions.ow, C) and tuple(cmask.shape) == (n * Bm, regions.oh, regions.ow)
            for i in range(n):                                         # crop_resample per region, bit for bit
                want_img, want_mask = detail.crop_resample(dev[0], masks[i].to(DEV), regions.region(i), "bilinear")
                assert np.array_equal(_bits(cimg[i * B:(i + 1) * B]), _bits(want_img)), (what, i, "image")
                assert np.array_equal(_bits(cmask[i * Bm:(i + 1) * Bm]), _bits(want_mask)), (what, i, "mask")
        return Case((image.numpy(), mask.numpy(), labels), lambda i, m, lab: detail.crop_regions(i, m, regions, lab, "bilinear"), check,
                    launches=lambda names, chunked: _only(names, lp_detail_resample_regions=2))
    assert call == "stitch_regions"
    return Case((image.numpy(), det.numpy(), mask.numpy(), labels),
                lambda o, d, m, lab: detail.stitch_regions(o, d, m, regions, lab, K, "bilinear"),
                lambda got, dev, what: _regions_stitch_check(got, dev[0], dev[1], image, det, mask, labels, regions, masks, what),
                launches=lambda names, chunked: _only(names, lp_detail_resample=1, lp_detail_stitch_regions=1))


@functools.lru_cache(maxsize=None)
def _track_scene(plane, C):
    H, W = plane
    image, mask = torch.rand(CLIP, H, W, C, generator=_gen(H, W, C, 5)), _two_subjects(H, W, empty=1)
    boxes = image_inputs._boxes_ref(mask)
    assert boxes[1] == (H, -1, W, -1) and all(b[1] >= 0 for f, b in enumerate(boxes) if f != 1)   # the empty frame's row is written
    track = detail.plan_track(boxes, H, W, 1.0, 1, 2, 2 * TARGET, smooth=3)
    assert track.resampled and len(set(track.origins)) > 1
    det = torch.rand(CLIP, track.oh, track.ow, C, generator=_gen(H, W, C, 6))
    return image, mask, boxes, track, det


def _track_stitch_check(got, dev_original, dev_det, dev_mask, original, track, what):
    """tests/test_gpu_detail_track.py's: `stitch` frame by frame bit for bit, and the outside of every window left alone."""
    for f in range(CLIP):
        want = detail.stitch(dev_original[f:f + 1], dev_det[f:f + 1], dev_mask[f:f + 1], track.region(f), K, FILTER)
        assert np.array_equal(_bits(got[f:f + 1]), _bits(want)), (what, f)
    outside = ~image_checks._window_mask(track)
    assert bool(outside.flatten(1).any(dim=1).all()) and np.array_equal(_bits(got.cpu()[outside]), _bits(original[outside])), what


@functools.lru_cache(maxsize=None)
def _detail_track(plane, C, Bm, mode, call):
    image, mask, boxes, track, det = _track_scene(plane, C)
    if call == "mask_bbox_frames":
        def check(got, dev, what):
            assert got == boxes, (what, got, boxes)
        return Case((mask.numpy(),), detail.mask_bbox_frames, check, launches=lambda names, chunked: _only(names, lp_mask_bbox_frames=1))
    if call == "crop_track":
        def check(got, dev, what):
            cimg, cmask = got
            assert tuple(cimg.shape) == (CLIP, track.oh, track.ow, C) and tuple(cmask.shape) == (CLIP, track.oh, track.ow)
            for f in range(CLIP):                                      # crop_resample per frame, bit for bit
                want_img, want_mask = detail.crop_resample(dev[0][f:f + 1], dev[1][f:f + 1], track.region(f), FILTER)
                assert np.array_equal(_bits(cimg[f:f + 1]), _bits(want_img)), (what, f, "image")
                assert np.array_equal(_bits(cmask[f:f + 1]), _bits(want_mask)), (what, f, "mask")
        return Case((image.numpy(), mask.numpy()), lambda i, m: detail.crop_track(i, m, track, FILTER), check,
                    launches=lambda names, chunked: _only(names, lp_detail_resample_track=2))
    assert call == "stitch_track"
    return Case((image.numpy(), det.numpy(), mask.numpy()), lambda o, d, m: detail.stitch_track(o, d, m, track, K, FILTER),
                lambda got, dev, what: _track_stitch_check(got, dev[0], dev[1], dev[2], image, track, what),
                launches=lambda names, chunked: _only(names, lp_detail_resample=1, lp_detail_stitch_track=1))


@functools.lru_cache(maxsize=None)
def _subjects_scene(plane, C):
    H, W = plane
    image, mask = torch.rand(CLIP, H, W, C, generator=_gen(H, W, C, 7)), _two_subjects(H, W)
    labels, n, table = subjects_ref.label_frames_ref(mask.numpy() > 0.5)
    table = tuple(tuple(int(v) for v in row) for row in table)
    assert n == len(BLOBS) and all(row[:2] == (0, CLIP - 1) for row in table)
    members = detail_subjects.group_subjects((n, table))
    boxes = tuple(tuple(tuple(int(v) for v in box) for box in sub) for sub in subjects_ref.subject_boxes_ref(labels, members))
    sub = detail_subjects.plan_subjects(members, boxes, H, W, 1.0, 1, 2, TARGET, 3)
    assert sub.subjects == n and sub.frames == CLIP and sub.resampled and sub.members == ((1,), (2,))
    det = torch.rand(n * CLIP, sub.oh, sub.ow, C, generator=_gen(H, W, C, 8))
    return image, mask, labels, n, table, members, boxes, sub, det


def _subjects_stitch_check(got, dev_original, dev_det, original, det, mask, labels, sub, what):
    """tests/test_gpu_detail_subjects.py's: the composition of `stitch` over subjects and frames bit for bit, and the torch
    restatement."""
    out = dev_original.clone()
    for s in range(sub.subjects):
        ms = subjects_ref.subject_mask(mask, labels, sub.members[s]).to(DEV)
        for f in range(CLIP):
            i = s * CLIP + f
            out[f:f + 1] = detail.stitch(out[f:f + 1].contiguous(), dev_det[i:i + 1], ms[f:f + 1], sub.window(s, f), K, "bilinear")
    assert np.array_equal(_bits(got), _bits(out)), what
    cover = int(subjects_ref.cover_count(sub).max())
    err = float((got.cpu() - subjects_ref.stitch_subjects_ref(original, det, mask, sub, labels, K, "bilinear")).abs().max())
    assert err <= cover * _stitch_bound(sub, "bilinear", det), (what, err)


@functools.lru_cache(maxsize=None)
def _detail_subjects(plane, C, Bm, mode, call):
    image, mask, labels, n, table, members, boxes, sub, det = _subjects_scene(plane, C)
    if call == "mask_components_frames":
        def check(got, dev, what):
            got_labels, got_n, got_table = got
            assert got_labels.is_cuda and got_labels.dtype == torch.int32 and got_n == n, (what, got_n)
            assert np.array_equal(got_labels.cpu().numpy(), labels) and got_table == table, what
        return Case((mask.numpy(),), detail_subjects.mask_components_frames, check,
                    launches=lambda names, chunked: _only(names, lp_mask_components_frames=1))
    if call == "subject_boxes":
        def check(got, dev, what):
            assert got == boxes, (what, got, boxes)
        return Case((labels,), lambda lab: detail_subjects.subject_boxes(lab, members), check,
                    launches=lambda names, chunked: _only(names, lp_subject_boxes=1))
    if call == "crop_subjects":
        def check(got, dev, what):
            cimg, cmask = got
            assert tuple(cimg.shape) == (n * CLIP, sub.oh, sub.ow, C) and tuple(cmask.shape) == (n * CLIP, sub.oh, sub.ow)
            for s in range(n):                                         # crop_resample per subject and frame, bit for bit
                ms = subjects_ref.subject_mask(mask, labels, sub.members[s]).to(DEV)
                for f in range(CLIP):
                    wimg, wmask = detail.crop_resample(dev[0][f:f + 1], ms[f:f + 1], sub.window(s, f), "bilinear")
                    assert np.array_equal(_bits(cimg[s * CLIP + f]), _bits(wimg[0])), (what, s, f, "image")
                    assert np.array_equal(_bits(cmask[s * CLIP + f]), _bits(wmask[0])), (what, s, f, "mask")
        return Case((image.numpy(), mask.numpy(), labels), lambda i, m, lab: detail_subjects.crop_subjects(i, m, sub, lab, "bilinear"),
                    check, launches=lambda names, chunked: _only(names, lp_detail_resample_subjects=2))
    assert call == "stitch_subjects"
    return Case((image.numpy(), det.numpy(), mask.numpy(), labels),
                lambda o, d, m, lab: detail_subjects.stitch_subjects(o, d, m, sub, lab, K, "bilinear"),
                lambda got, dev, what: _subjects_stitch_check(got, dev[0], dev[1], image, det, mask, labels, sub, what),
                launches=lambda names, chunked: _only(names, lp_detail_resample=1, lp_detail_stitch_subjects=1))


# ---- A: every public call under 0x00 and 0xFF ---------------------------------------------------------------------------------------------------
# name -> (builder, further arguments, kind, chunked too).  Kinds: "image" runs on CONFIGS; "mask" has no image (C = 0) and "clip"
# brings a mask per frame of its own: both planes; "audio" is (samples, 0, 0): one under and one at a multiple of the float4.
CALLS = {
    "mask_blend": (_mask_blend, (), "image", False),
    "merge_video_with_mask": (_merge_video, (False,), "image", False),
    "merge_video_with_mask[half-resolution mask]": (_merge_video, (True,), "image", False),
    "merge_audio_with_mask": (lambda n, C, Bm, mode: _merge_audio(n), (), "audio", False),
    "interpolate_masks": (_interpolate_masks, (), "clip", False),
    "mask_bbox": (_detail_single, ("mask_bbox",), "image", False),
    "crop_resample": (_detail_single, ("crop_resample",), "image", False),
    "stitch": (_detail_single, ("stitch",), "image", False),
    "mask_components": (_detail_regions, ("mask_components",), "image", False),
    "crop_regions": (_detail_regions, ("crop_regions",), "image", False),
    "stitch_regions": (_detail_regions, ("stitch_regions",), "image", False),
    "mask_bbox_frames": (_detail_track, ("mask_bbox_frames",), "clip", False),
    "crop_track": (_detail_track, ("crop_track",), "clip", False),
    "stitch_track": (_detail_track, ("stitch_track",), "clip", False),
    "mask_components_frames": (_detail_subjects, ("mask_components_frames",), "clip", False),
    "subject_boxes": (_detail_subjects, ("subject_boxes",), "clip", False),
    "crop_subjects": (_detail_subjects, ("crop_subjects",), "clip", False),
    "stitch_subjects": (_detail_subjects, ("stitch_subjects",), "clip", False),
    "detail_color.match[mean_std]": (_color_match, ("mean_std",), "image", False),
    "detail_color.match[mean]": (_color_match, ("mean",), "image", False),
    "fill_masked": (_fill_masked, (), "image", False),
    "outpaint_pad[fill, mask]": (_outpaint_pad, (True, True), "image", False),
    "outpaint_pad[fill, no mask]": (_outpaint_pad, (True, False), "image", False),
    "outpaint_pad[no fill, mask]": (_outpaint_pad, (False, True), "image", False),
    "outpaint_pad[no fill, no mask]": (_outpaint_pad, (False, False), "image", False),
    "blend_multiband": (_blend_multiband, (), "image", True),
    "grow_mask[+3]": (_grow_mask, (3,), "mask", True),
    "grow_mask[-3]": (_grow_mask, (-3,), "mask", True),
    "refine_mask[radius 8]": (_refine_mask, (8, 0), "image", True),
    "refine_mask[radius 8, grow 2]": (_refine_mask, (8, 2), "image", True),
    "refine_mask[radius 0, grow 2]": (_refine_mask, (0, 2), "image", True),
    "refine_mask[radius 0, grow 0]": (_refine_mask, (0, 0), "image", False),
    "refine_mask[radius 64]": (_refine_mask, (64, 0), "small", True),   # the window wider than the image
    "stabilize_masks": (_stabilize_masks, (), "video", True),
    "grain.match": (_grain_match, (False, 0), "image", True),
    "grain.match[clip_frames 3]": (_grain_match, (False, 3), "image", True),
    "grain.match[reference]": (_grain_match, (True, 0), "image", True),
    "grain.match[reference, clip_frames 3]": (_grain_match, (True, 3), "image", True),
}
KINDS = {"image": CONFIGS, "small": CONFIGS[:1], "mask": [(SMALL, 0, 1), (LARGE, 0, B)], "clip": [(SMALL, 3, 0), (LARGE, 3, 0), (LARGE, 4, 0)],
         "video": [(SMALL, 0, 0), (LARGE, 0, 0)], "audio": [(3001, 0, 0), (4000, 0, 0)]}
KINDS_CHUNKED = {"image": CHUNKED, "small": CHUNKED[:1], "mask": [(SMALL, 0, B), (LARGE, 0, B)], "video": KINDS["video"]}
CLIP_MASK_ONLY = ("interpolate_masks", "mask_bbox_frames", "mask_components_frames", "subject_boxes")       # these read no image


def _case(name, plane, C, Bm, mode):
    builder, more, _, _ = CALLS[name]
    return builder(plane, C, Bm, mode, *more)


def _cases():
    out = []
    for name, (_, _, kind, chunked) in CALLS.items():
        configs = [c for c in KINDS[kind] if not (name in CLIP_MASK_ONLY and c[1] == 4)]
        out += [(name, *c, "whole") for c in configs]
        if chunked:
            out += [(name, *c, "chunked") for c in KINDS_CHUNKED[kind]]
    return out


def _case_id(c):
    name, plane, C, Bm, mode = c
    shape = "x".join(map(str, plane)) if isinstance(plane, tuple) else str(plane)
    return f"{name}-{shape}-C{C}-M{Bm}-{mode}"


CASES = _cases()


@pytest.mark.parametrize("poison", POISONS, ids=poison_id)
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_the_call_under_poison_meets_its_suites_comparison(case, poison, monkeypatch):
    name, plane, C, Bm, mode = case
    this = _case(*case)
    dev = this.device()
    if mode == "chunked":
        this.caps(monkeypatch)
    names = record_launches(monkeypatch, *MODULES)
    filled = poisoned_empty(monkeypatch, poison)
    got = this.run(*dev)
    launched = list(names)
    assert bool(filled) == this.allocates, (case, filled)               # the call's buffers did come through the poison
    if this.launches is not None:
        this.launches(launched, mode == "chunked")
    this.check(got, dev, (*case, poison_id(poison)))


def test_chunked_mode_takes_more_chunks_than_whole_mode(monkeypatch):
    """Without this the lowered caps of the chunked cases above proved nothing: every module that has a cap launches its chunked
    entry more often under it, on both planes."""
    for name, (_, _, kind, chunked) in CALLS.items():
        if not chunked:
            continue
        for config in KINDS_CHUNKED[kind]:
            counts = {}
            for mode in ("whole", "chunked"):
                this = _case(name, *config, mode)
                with monkeypatch.context() as patch:
                    if mode == "chunked":
                        this.caps(patch)
                    names = record_launches(patch, *MODULES)
                    this.run(*this.device())
                    counts[mode] = len(names)
            assert counts["chunked"] > counts["whole"], (name, config, counts)


# ---- A: the stage functions that allocate their own results, fed as their suites feed them, at (23, 33) -------------------------------------------
H, W = SMALL
stage = pytest.mark.parametrize("poison", POISONS, ids=poison_id)


@stage
def test_keyframe_edt_under_poison(poison, monkeypatch):
    filled = poisoned_empty(monkeypatch, poison)
    rng = np.random.default_rng(11)
    masks = [(rng.random((H, W)) < p).astype(np.float32) for p in (0.002, 0.05, 0.5, 0.97)]
    masks += [rng.random((H, W)).astype(np.float32), np.zeros((H, W), np.float32), np.ones((H, W), np.float32)]
    image_checks._check_edt(masks)                                          # d2 of both planes, the centroid sums and the SDF, exactly
    assert filled


@stage
def test_morph_frames_and_resize_codes_under_poison(poison, monkeypatch):
    filled = poisoned_empty(monkeypatch, poison)
    rng = np.random.default_rng(100 * H + W)
    keys = image_inputs._keys(rng, H, W)
    stack = device._dev(keys)
    _, sdf, _ = videomask.keyframe_edt(stack)
    plan, _, _ = image_checks._hand_plan(H, W, len(keys))
    _, codes, _ = image_checks._check_morph("poison", keys, stack, sdf, plan)                    # the float form and the codes
    for size in ((W + 17, H + 9), (W - 10, H), (20, 50)):
        got = videomask.resize_codes(device._dev(codes), size).cpu().numpy()
        assert np.array_equal(got, vref.pil_resize_ref(codes, size)), size
    assert filled


@stage
def test_color_stats_fit_and_apply_under_poison(poison, monkeypatch):
    filled = poisoned_empty(monkeypatch, poison)
    for C, Bm in ((3, B), (4, 1), (5, 1)):                             # 5: two channel groups
        (d, r), mask = image_inputs._images(B, H, W, C, 1), image_inputs._blob_mask(Bm, H, W, 2)
        stats = image_checks._check_color_stats(d, r, mask, MARGIN, ("stats", C))
        image_checks._check_color_stats(d, r, None, 0, ("no mask", C))
        for args in (("mean_std", 1.0, 1, 0), ("mean", 0.3, 3, 0), ("mean_std", 1.0, 0, 1), ("mean_std", 1.0, 3, 3)):
            coef = image_checks._fit_bits(stats, *args)
        got = detail_color.color_apply(_dev(d), _dev(coef))
        _same_bits(got, color_ref.apply_ref(d, coef), ("apply", C))
    assert filled


@stage
def test_signed_d2_and_stabilize_q_under_poison(poison, monkeypatch):
    filled = poisoned_empty(monkeypatch, poison)
    for name in ("soft", "blobs"):
        mask = image_inputs.FORMS[name](FRAMES, H, W)
        q_ref = sref.signed_d2(mask)
        q_dev = image_checks._device_q(mask)
        assert q_dev.dtype == torch.int32 and (q_dev.cpu().numpy() == q_ref).all(), name
        image_checks._check_q(q_dev, q_ref, [(0, 0, 0.0, 0.0), (1, 2, 0.0, 0.0), (2, 1, 0.5, 3.0), (3, 8, -0.5, 0.5)], name)
    assert filled


@stage
def test_grain_stats_fit_field_and_apply_under_poison(poison, monkeypatch):
    filled = poisoned_empty(monkeypatch, poison)
    C = 3
    image, mask = _grain_scene(SMALL, C, B, "whole")
    cases = [("all", 64, 8), ("outside", 64, 2), ("inside", 64, 8)]    # the three regions
    got = image_checks._check_grain_stats(image, mask, cases, "stats")
    assert all(g[..., 0].sum() > 0 and (g[..., 0] == 0).any() for g in got)        # measured, and bands that nothing touched
    gen, plate = image_inputs._random_table(B, C, 1, 100), image_inputs._random_table(5, C, 3)
    image_checks._check_fit(gen, image_inputs._random_table(B, C, 2), [(1.0, -1, 0), (1.0, -1, 1), (0.8, -1, 3), (1.3, 1, 3)], "fit")
    image_checks._check_fit(gen, plate, [(1.0, -1, 0), (1.0, 2, 3)], "fit, plate")
    for size in (0, 1, 2):
        field = grain.grain_field((B, H, W, C), size, 21, size == 1, 7, DEV).cpu().numpy()
        compare._same_typed(field, gref.grain_field(B, H, W, C, size, 21, size == 1, 7), ("field", size))
    amp = (image_inputs._named_rng("poison", 7).random((B, C, gref.K)) * 3e-4).astype(np.float32)
    amp[0, 0, 3] = 0.0
    sizes = np.array([0, 2, 1], np.int32)
    out = grain.grain_apply(_dev(image), _dev(mask), _dev(amp), _dev(sizes), seed=4, frame0=1000).cpu().numpy()
    compare._same_typed(out, gref.grain_apply(image, mask, amp, sizes, 4, False, 1000), "apply")
    assert filled


@stage
def test_reshape_mask_under_poison(poison, monkeypatch):
    """lanpaint_amd/resample.py's one entry, through nodes.reshape_mask as tests/test_gpu_kernels.py feeds it."""
    from lanpaint_amd.nodes import reshape_mask
    filled = poisoned_empty(monkeypatch, poison)
    rng = np.random.default_rng(17)
    for src_shape, out_shape, video in (((9, H, W), (1, 4, 3, 5, 7), True), ((H, W), (2, 4, 8, 8), False), ((3, H, W), (3, 4, 5, 3), False)):
        m = (rng.random(src_shape) > 0.7).astype(np.float32)
        got = reshape_mask(_dev(m), out_shape, video_inpainting=video)
        assert tuple(got.shape) == tuple(out_shape)
        assert np.array_equal(got.cpu().numpy(), orc.reshape_mask(m, out_shape, video_inpainting=video)), (src_shape, out_shape)
    assert filled


# ---- B: off the null stream, behind a delay ---------------------------------------------------------------------------------------------------
# How long the side stream is held back, in milliseconds.  It has to outlast the host's side of the call.  Measured on the MI355X
# (the warm call of each call of the first group on (23, 33), whole mode, host wall time in ms; the call behind the delay, which
# also fills its buffers with 0xFF, took about 0.05 ms more):
#     fill_masked 0.03, outpaint_pad 0.05, blend_multiband 0.08, refine_mask (radius 8, grow 2) 0.10, refine_mask (radius 0, grow 2)
#     0.08, grow_mask 0.07, stabilize_masks 0.05, detail_color.match 0.04, grain.match 0.07 (with a reference 0.07), mask_blend 0.02,
#     merge_video_with_mask 0.02, merge_audio_with_mask 0.04
# The largest is 0.10 ms, 0.15 ms under the poison.  Twenty times that would be 3 ms; the motion family's 100 ms is kept, more
# than 600 times the largest, for the shared machine's host jitter, and the thirteen tests still wait 1.3 s in all.
DELAY_MS = 100


def _held_back(side, monkeypatch):
    """On `side`, the current stream: queue the delay and the event behind it; -> (event, the list the 0xFF poison fills)."""
    filled = poisoned_empty(monkeypatch, 0xFF)
    done = torch.cuda.Event()
    torch.cuda._sleep(int(_spin_cycles_per_ms() * DELAY_MS))
    done.record(side)
    return done, filled


def _side_config(name):
    return KINDS[CALLS[name][2]][0]


# The calls whose docstrings say "no device -> host read" (fill_masked, blend_multiband, refine_mask, grow_mask, stabilize_masks,
# detail_color.match, grain.match; fill.py says it of outpaint_pad too), and the three that state nothing.
NO_READ = ["fill_masked", "outpaint_pad[fill, mask]", "blend_multiband", "refine_mask[radius 8, grow 2]", "refine_mask[radius 0, grow 2]",
           "grow_mask[+3]", "stabilize_masks", "detail_color.match[mean_std]", "grain.match", "grain.match[reference, clip_frames 3]",
           "mask_blend", "merge_video_with_mask[half-resolution mask]", "merge_audio_with_mask"]


@pytest.mark.parametrize("name", NO_READ)
def test_the_call_on_a_held_back_side_stream_reads_nothing_back(name, monkeypatch):
    """tests/test_gpu_motion_scratch.py's test of the same name, for the image-space calls: made on a side stream that is still
    busy with a delay queued in front of it, the call returns before the delay is done (no device -> host read, no
    synchronisation -- and the delay did outlast the host's side of the call: were it too short, this fails rather than proving
    nothing), leaves nothing on the null stream, and every launch, copy and memset waits on that stream behind the 0xFF fills
    of its buffers, or the bits differ."""
    this = _case(name, *_side_config(name), "whole")
    dev = this.device()                                                # built on the default stream
    _spin_cycles_per_ms()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        this.run(*dev)                                                 # the first call loads the kernels and fills the allocator's
        side.synchronize()                                             # pool of this stream: no hipMalloc below
        start = time.perf_counter()
        warm = this.run(*dev)
        warm_ms = (time.perf_counter() - start) * 1e3
        del warm
        side.synchronize()
        done, filled = _held_back(side, monkeypatch)
        start = time.perf_counter()
        got = this.run(*dev)
        held = not done.query()                                        # directly behind the call, before anything synchronises
        idle = torch.cuda.default_stream().query()
        call_ms = (time.perf_counter() - start) * 1e3
        print(f"IMAGE_SIDE {name}: warm call {warm_ms:.2f} ms, call behind the delay {call_ms:.2f} ms of host time; delay {DELAY_MS} ms")
        assert held, (f"{name} returned after {call_ms:.2f} ms with the {DELAY_MS} ms delay in front of it done: it waited for the "
                      "device, or the delay is too short for this host")
        assert idle, f"{name} left work on the null stream"
        assert filled
        side.synchronize()
        this.check(got, dev, (name, "side stream"))


def _count_reads(monkeypatch):
    """The list that gets one entry per `.cpu()`, `.item()`, `.tolist()` and `.numpy()` made on a HIP tensor from here on."""
    reads = []
    for method in ("cpu", "item", "tolist", "numpy"):
        def counted(self, *args, _real=getattr(torch.Tensor, method), _name=method, **kwargs):
            if self.is_cuda:
                reads.append(_name)
            return _real(self, *args, **kwargs)
        monkeypatch.setattr(torch.Tensor, method, counted)
    return reads


def _chain_single(dev):
    """The single form as detail_nodes composes it; the crop goes back as the detailed crop."""
    image, mask = dev
    H, W = image.shape[1:3]
    region = detail.plan_region(detail.mask_bbox(mask), H, W, 1.0, 1, 8, 2 * TARGET)
    cimg, cmask = detail.crop_resample(image, mask, region, FILTER)
    return region, cimg, cmask, detail.stitch(image, cimg, mask, region, K, FILTER)


def _chain_regions(dev):
    image, mask = dev
    H, W = image.shape[1:3]
    labels, n, table = detail.mask_components(mask)
    regions = detail.plan_regions((n, table), H, W, 1.0, 1, 2, TARGET)
    cimg, cmask = detail.crop_regions(image, mask, regions, labels, "bilinear")
    return regions, cimg, cmask, detail.stitch_regions(image, cimg, mask, regions, labels, K, "bilinear")


def _chain_track(dev):
    image, mask = dev
    H, W = image.shape[1:3]
    track = detail.plan_track(detail.mask_bbox_frames(mask), H, W, 1.0, 1, 2, 2 * TARGET, smooth=3)
    cimg, cmask = detail.crop_track(image, mask, track, FILTER)
    return track, cimg, cmask, detail.stitch_track(image, cimg, mask, track, K, FILTER)


def _chain_subjects(dev):
    image, mask = dev
    H, W = image.shape[1:3]
    labels, n, table = detail_subjects.mask_components_frames(mask)
    members = detail_subjects.group_subjects((n, table))
    sub = detail_subjects.plan_subjects(members, detail_subjects.subject_boxes(labels, members), H, W, 1.0, 1, 2, TARGET, 3)
    cimg, cmask = detail_subjects.crop_subjects(image, mask, sub, labels, "bilinear")
    return sub, cimg, cmask, detail_subjects.stitch_subjects(image, cimg, mask, sub, labels, K, "bilinear")


def _check_chain(form, got, dev):
    """The windows are the scene's own, the crop meets its form's comparison and the stitch of that crop its form's."""
    win, cimg, cmask, out = got
    det = cimg.cpu()
    if form == "single":
        image, mask, _, region, _ = _single_scene(SMALL, 3, 1)
        assert win == region
        _resample_check(cimg, image, region, FILTER, "chain")
        _single_stitch_check(out, image, det, mask, region, "chain")
    elif form == "regions":
        image, mask, labels, _, _, regions, masks, _ = _regions_scene(SMALL, 3, 1)
        assert win == regions
        _regions_stitch_check(out, dev[0], cimg, image, det, mask, labels, regions, masks, "chain")
    elif form == "track":
        image, mask, _, track, _ = _track_scene(SMALL, 3)
        assert win == track
        _track_stitch_check(out, dev[0], cimg, dev[1], image, track, "chain")
    else:
        image, mask, labels, _, _, _, _, sub, _ = _subjects_scene(SMALL, 3)
        assert win == sub
        _subjects_stitch_check(out, dev[0], cimg, image, det, mask, labels, sub, "chain")


def _scene_inputs(form):
    scene = {"single": lambda: _single_scene(SMALL, 3, 1), "regions": lambda: _regions_scene(SMALL, 3, 1),
             "track": lambda: _track_scene(SMALL, 3), "subjects": lambda: _subjects_scene(SMALL, 3)}[form]()
    return scene, (_dev(scene[0].numpy()), _dev(scene[1].numpy()))


def _both_subject_reads(dev):
    labels, n, table = detail_subjects.mask_components_frames(dev[0])
    return (labels, n, table), detail_subjects.subject_boxes(labels, detail_subjects.group_subjects((n, table)))


# name -> (the reads its docstring states, how it runs).  A reading call cannot return before the delay is done: the read waits
# for it.  What holds instead: the null stream is idle, the comparison passes, and the reads are as many as the docstring says.
READING = {
    "mask_bbox": 1, "mask_components": 1, "mask_bbox_frames": 1, "mask_components_frames + subject_boxes": 2, "interpolate_masks": 1,
    "single": 1, "regions": 1, "track": 1, "subjects": 2,
}


@pytest.mark.parametrize("name", list(READING))
def test_the_reading_call_on_a_held_back_side_stream_reads_as_often_as_its_docstring_says(name, monkeypatch):
    """detail.py: "the job's one device -> host read" of each of its three forms; detail_subjects.py: the "first" and the "second
    and last"; videomask.interpolate_masks: the centroid sums, once.  The crop -> stitch chains are composed as the nodes
    compose them."""
    chain = name in ("single", "regions", "track", "subjects")
    if chain:
        _, dev = _scene_inputs(name)
        run = {"single": _chain_single, "regions": _chain_regions, "track": _chain_track, "subjects": _chain_subjects}[name]
        run = functools.partial(run, dev)
        check = lambda got: _check_chain(name, got, dev)                # noqa: E731
    elif name == "mask_components_frames + subject_boxes":
        first, second = (_case(n, SMALL, 3, 0, "whole") for n in ("mask_components_frames", "subject_boxes"))
        dev = first.device()
        run = functools.partial(_both_subject_reads, dev)
        check = lambda got: (first.check(got[0], dev, name), second.check(got[1], dev, name))      # noqa: E731
    else:
        this = _case(name, *_side_config(name), "whole")
        dev = this.device()
        run = functools.partial(this.run, *dev)
        check = lambda got: this.check(got, dev, (name, "side stream"))   # noqa: E731
    _spin_cycles_per_ms()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        run()
        side.synchronize()
        done, filled = _held_back(side, monkeypatch)
        reads = _count_reads(monkeypatch)
        got = run()
        counted = list(reads)
        idle = torch.cuda.default_stream().query()
        assert idle, f"{name} left work on the null stream"
        assert filled
        side.synchronize()
        assert len(counted) == READING[name], (name, counted)
        check(got)


@pytest.mark.parametrize("first_on", ["default", "side"])
def test_the_table_cache_serves_both_streams(first_on, monkeypatch):
    """`_util.device_tables` uploads a geometry's tap tables once for the process, on whichever stream was current.  The upload
    on the default stream and the launch on the held-back side stream, and the reverse: both calls give the bits of a call on
    one stream."""
    image, _, _, region, _ = _single_scene(SMALL, 3, 1)
    dev = _dev(image.numpy())
    crop = lambda: detail.crop_resample(dev, None, region, FILTER)[0]   # noqa: E731
    _util.device_tables.cache_clear()
    want = _bits(crop())
    _spin_cycles_per_ms()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        crop()                                                         # loads nothing new; fills the side stream's pool
        side.synchronize()
    _util.device_tables.cache_clear()
    assert _util.device_tables.cache_info().currsize == 0
    tables = len({(region.h, region.oh), (region.w, region.ow)})
    if first_on == "default":
        first = crop()
        torch.cuda.synchronize()
        assert _util.device_tables.cache_info().currsize == tables
    with torch.cuda.stream(side):
        done, filled = _held_back(side, monkeypatch)
        on_side = crop()                                               # first_on == "side": the upload waits behind the delay
    if first_on == "side":
        assert _util.device_tables.cache_info().currsize == tables
        first = crop()                                                 # on the default stream, from the side stream's upload
    assert filled
    torch.cuda.synchronize()
    assert _util.device_tables.cache_info().misses == tables
    assert np.array_equal(_bits(first), want) and np.array_equal(_bits(on_side), want)
