"""The video mask kernels (csrc/videomask_kernel.hip, csrc/resample_tile.h) on the MI355X against live references, beyond the
recorded fixtures: lp_vmask_resize bit for bit against live Pillow at the sizes, tap counts and tile edges the fixtures do not
reach; lp_vmask_morph against the float64 arbiter (tests/videomask_ref.py, pinned bit for bit to all fixtures by
tests/test_videomask_host.py) on hand-built plans; lp_vmask_edt exactly, at the sides where the row pass opts in to more
than 64 KiB of LDS; and interpolate_masks end to end.  Every comparison covers every output element."""
import ctypes

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, videomask
from lanpaint_amd._util import raw_stream
from lanpaint_amd.videomask import FRAME_DTYPE, frame_plan
from tests import videomask_ref as vref
from tests.device import DEV, _dev
from tests.image_checks import PLAN_INNER as INNER, PLAN_KEY as KEY, PLAN_ZERO as ZERO, _check_morph, _hand_plan
from tests.image_inputs import _apply, _blob, _keys, _pairs, _row

pytestmark = pytest.mark.gpu
NONE = _cabi.LP_VMASK_D2_NONE


# ---- resize: live Pillow, bit for bit ------------------------------------------------------------------------------------------
def _resize_pairs():
    pairs = list(_pairs())                                               # the 32 the host model is held to
    pairs += [((3840, 2160), (480, 270)),                                # ksize 17 on both axes
              ((1920, 1080), (1920, 540)), ((1920, 1080), (960, 1080)),  # one axis only: the other pass is an identity
              ((16384, 9), (2048, 9)),                                   # the widest source, eight 256-element tiles
              ((1000, 16384), (1000, 300)),                              # ksize 111, about 31 LDS chunks per tile
              ((5, 3), (16384, 1)), ((300, 2), (1, 1))]
    pairs += [((300, 24), (ow, 19)) for ow in (255, 256, 257, 258, 260, 1023)]   # vector store, scalar store, scalar last tile
    pairs += [((56, 40), (97, oh)) for oh in (15, 16, 17, 33)]                    # the 16-row tile's edge
    seen, out = set(), []
    for p in pairs:
        if p not in seen:
            seen.add(p)
            out.append(p)
    return out


def _random_codes(rng, h, w):
    codes = rng.integers(0, 256, (h, w), dtype=np.uint8)
    codes[rng.random((h, w)) < 0.5] = 0                                  # masks: flat regions and edges
    return codes


def _contents(rng, h, w):
    yy, xx = np.mgrid[:h, :w]
    corners = np.zeros((h, w), np.uint8)
    corners[[0, 0, -1, -1], [0, -1, 0, -1]] = 255
    return {"random": _random_codes(rng, h, w),
            "all255": np.full((h, w), 255, np.uint8),                    # rounded weights can sum past 1 << 22: clip8 saturates
            "all0": np.zeros((h, w), np.uint8),
            "checker": (((yy + xx) & 1) * 255).astype(np.uint8),
            "corners": corners}


def _resize(codes, size):
    out = videomask.resize_codes(_dev(codes), size)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("src,dst", _resize_pairs(), ids=lambda p: f"{p[0]}x{p[1]}")
def test_resize_equals_live_pillow(src, dst):
    pytest.importorskip("PIL.Image")
    (w, h), (ow, oh) = src, dst
    rng = np.random.default_rng(w * 1000 + h)
    c = _contents(rng, h, w)
    for name, frame in c.items():                                        # F = 1
        got = _resize(frame[None], (ow, oh))
        assert got.shape == (1, oh, ow) and got.dtype == np.float32
        assert np.array_equal(got, vref.pil_resize_ref(frame[None], (ow, oh))), name
    stack = np.stack([c["random"], c["all255"], _random_codes(rng, h, w), c["checker"], c["all0"], c["corners"],
                      _random_codes(rng, h, w)])                         # F = 7, every frame its own image: the frame strides
    got = _resize(stack, (ow, oh))
    want = vref.pil_resize_ref(stack, (ow, oh))
    assert got.shape == want.shape == (7, oh, ow)
    for f in range(7):
        assert np.array_equal(got[f], want[f]), f


def _overshooting_table(rng, in_size, out_size):
    """A tap table no bilinear resize produces: one or two taps whose weights sum to 1.5, 1, 0.75 or -0.5."""
    choices = np.array([[1 << 22, 1 << 21], [1 << 22, 0], [3 << 20, 0], [-(1 << 21), 0], [1 << 21, 1 << 21]], np.int32)
    bounds = np.zeros((out_size, 2), np.int32)
    bounds[:, 0] = rng.integers(0, in_size - 1, out_size)
    bounds[:, 1] = 2
    weights = choices[rng.integers(0, len(choices), out_size)]
    weights[0], bounds[0] = choices[0], (0, 2)                           # output 0: 1.5 times the first two source pixels
    return bounds, np.ascontiguousarray(weights)


def test_resize_saturates_as_pillow_clip8_does():
    """Pillow's clip8 at both ends, in both passes.  Normalised bilinear weights cannot reach the upper end from uint8 codes
    (255 * sum(w) stays below 256 << 22 for any rounding excess of a few units), so the tables here are hand-built and go
    through the C entry directly; the arbiter is the two integer passes of tests/test_videomask_host.py, which are held to
    live Pillow.  A horizontal sum that is not clipped would spill into the neighbouring byte of the packed staging."""
    rng = np.random.default_rng(8)
    h, w, oh, ow = 40, 300, 23, 270
    codes = _random_codes(rng, h, w)
    codes[:8, :16] = 255
    codes[rng.random((h, w)) < 0.3] = 255
    bx, kx = _overshooting_table(rng, w, ow)
    by, ky = _overshooting_table(rng, h, oh)
    want = _apply(codes, bx, kx, by, ky)
    assert want[0, 0] == 255 and (want == 255).mean() > 0.05 and (want == 0).mean() > 0.05
    assert ((want > 0) & (want < 255)).mean() > 0.05
    src, out = _dev(codes[None]), torch.empty((1, oh, ow), dtype=torch.float32, device=DEV)
    tables = [_dev(t) for t in (bx, kx, by, ky)]
    d = _cabi.LpVmaskResizeDesc(1, h, w, oh, ow, 2, 2, 0, src.data_ptr(), *(t.data_ptr() for t in tables), out.data_ptr())
    with torch.cuda.device(DEV):
        _cabi.check(_cabi.load().lp_vmask_resize(ctypes.byref(d), raw_stream(DEV)), "lp_vmask_resize")
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy()[0], want.astype(np.float32) / np.float32(255))

# ---- morph: the float64 arbiter ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(1, 1), (1, 300), (300, 1), (37, 53), (64, 64), (257, 1000), (480, 832)],
                         ids=lambda v: str(v))
def test_morph_equals_the_arbiter(h, w):
    pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(100 * h + w)
    keys = _keys(rng, h, w)
    n_keys = len(keys)
    stack = _dev(keys)
    _, sdf, csum = videomask.keyframe_edt(stack)
    want_sdf = np.stack([vref.sdf_ref(k) for k in keys])
    assert np.array_equal(sdf.cpu().numpy(), want_sdf)                   # so that a morph failure is the morph's
    assert (want_sdf[3] == -max(h, w) / 2.0).all() and (want_sdf[4] == max(h, w) / 2.0).all()

    indices, count = [1, 4, 5, 9, 13], 16                                # zero frames around, two adjacent keyframes
    centroids = [(sy / n, sx / n) if n else None for n, sy, sx in csum.cpu().tolist()]
    plan = frame_plan(indices, count, centroids)
    assert (plan["kind"] == INNER).sum() == 8 and centroids[3] is None  # 2 + 0 + 3 + 3 frames between the keyframes
    _check_morph("frame_plan", keys, stack, sdf, plan)

    plan, vacated, bad = _hand_plan(h, w, n_keys)
    got, codes, want = _check_morph("hand", keys, stack, sdf, plan)
    half = np.float32(0.5)
    for t in vacated:                                                    # v = 0 exactly: m = 0.5, code 127
        assert (got[t] == half).all() and (codes[t] == 127).all() and (want[t] == half).all(), t
    for t in bad:                                                        # nothing read, nothing but zeros written
        assert not got[t].any() and not codes[t].any() and not want[t].any(), t
    assert (got[19] == half).all() and (want[19] == half).all()         # empty to full at wf = 0.5: the halves cancel
    if (h, w) == (257, 1000):
        # wf = 0: v is key 0's SDF.  Beyond +-50 on both sides, so both clip branches ran: the sigmoid saturates to
        # exactly 1.0f above, and below it stops at float32(sigmoid(-50)) = 1.93e-22 (not 0: that is still a normal fp32;
        # without the clip exp would overflow and the result would be 0.0f).  The codes reach 0 and 255.
        v = want_sdf[0]
        assert (v > 50.0).any() and (v < -50.0).any()
        floor = np.float32(1.0 / (1.0 + np.exp(50.0)))
        assert got[12].max() == np.float32(1.0) and want[12].max() == np.float32(1.0)
        assert floor > 0 and want[12].min() == floor and vref.ulp_diff(got[12].min(), floor) <= 1
        assert (got[12][v > 50.0] == np.float32(1.0)).all()
        assert codes[12].max() == 255 and codes[12].min() == 0


def test_morph_without_an_sdf_writes_zero_inner_frames():
    """The documented form for plans without an inner frame: sdf = None; an INNER entry then reads nothing."""
    rng = np.random.default_rng(5)
    keys = _keys(rng, 37, 53)
    plan = np.array([_row(KEY, 1), _row(INNER, 0, 1, wf=0.5), _row(ZERO), _row(KEY, 4)], FRAME_DTYPE)
    got = videomask.morph_frames(_dev(keys), plan, None).cpu().numpy()
    assert np.array_equal(got[0], keys[1]) and not got[1].any() and not got[2].any() and np.array_equal(got[3], keys[4])


# ---- EDT at the sides where the row pass needs the LDS opt-in ------------------------------------------------------------------
def _brute_d2(target):
    """Squared distance to the nearest True pixel by brute force, a few target pixels at a time."""
    h, w = target.shape
    ys, xs = np.nonzero(target)
    yy, xx = np.mgrid[:h, :w]
    out = np.full((h, w), np.iinfo(np.int64).max, np.int64)
    step = max(1, (1 << 24) // (h * w))
    for c in range(0, len(ys), step):
        d = (yy[..., None] - ys[c:c + step]) ** 2 + (xx[..., None] - xs[c:c + step]) ** 2
        out = np.minimum(out, d.min(-1))
    return out


def _strip_masks(rng, h, w):
    """The contents of one strip: (name, float32 [h, w])."""
    corner = np.zeros((h, w), np.float32)
    corner[h - 1, w - 1] = 1.0                                           # the largest d2 of the strip is at (0, 0)
    column = np.zeros((h, w), np.float32)
    column[:, w // 3] = 1.0                                              # one parabola as wide as the row
    second = np.zeros((h, w), np.float32)
    second[:, ::2] = 1.0                                                 # the columns between never enter the envelope
    rows = np.zeros((h, w), np.float32)
    rows[::2, :] = 1.0                                                   # all-foreground rows next to all-background rows
    return [("sparse", (rng.random((h, w)) < 0.0005).astype(np.float32)),
            ("dense", (rng.random((h, w)) < 0.5).astype(np.float32)),
            ("corner", corner), ("column", column), ("second", second), ("rows", rows)]


def _check_strip(named):
    ndimage = pytest.importorskip("scipy.ndimage")
    masks = [m for _, m in named]
    d2, sdf, csum = videomask.keyframe_edt(_dev(np.stack(masks)))
    torch.cuda.synchronize()
    d2, sdf, csum = d2.cpu().numpy(), sdf.cpu().numpy(), csum.cpu().numpy()
    for k, (name, m) in enumerate(named):
        fg = m >= 0.5
        h, w = fg.shape
        for plane, target in ((0, fg), (1, ~fg)):
            got = d2[k, plane]
            if not target.any():
                assert (got == NONE).all(), (name, plane)
                continue
            dist = ndimage.distance_transform_edt(~target)               # exact: the sqrt of an integer
            assert np.array_equal(got, np.rint(dist * dist).astype(np.int64)), (name, plane)
            assert np.array_equal(np.sqrt(got.astype(np.float64)), dist), (name, plane)
            if np.count_nonzero(target) <= 256:
                assert np.array_equal(got, _brute_d2(target)), (name, plane)
        ys, xs = np.nonzero(fg)
        assert csum[k].tolist() == [len(ys), int(ys.sum()), int(xs.sum())], name
        assert np.array_equal(sdf[k], vref.sdf_ref(m)), name
        if name == "corner":
            yy, xx = np.mgrid[:h, :w]
            want = (yy - (h - 1)) ** 2 + (xx - (w - 1)) ** 2
            assert np.array_equal(d2[k, 0], want) and d2[k, 0, 0, 0] == (h - 1) ** 2 + (w - 1) ** 2
        if name == "column":
            assert np.array_equal(d2[k, 0], np.broadcast_to((np.arange(w) - w // 3) ** 2, (h, w)))
    return d2, sdf, csum


@pytest.mark.parametrize("w", [8190, 8191, 8192, 16384])                 # 8190: the last width without the opt-in
@pytest.mark.parametrize("h", [1, 5, 16])
def test_edt_wide_strips(h, w):
    _check_strip(_strip_masks(np.random.default_rng(h * 100000 + w), h, w))


@pytest.mark.parametrize("h", [16383, 16384])                            # the column pass, its 16-row unroll tail, far = H + W
@pytest.mark.parametrize("w", [1, 3])
def test_edt_tall_strips(h, w):
    _check_strip(_strip_masks(np.random.default_rng(h * 10 + w), h, w))


def test_edt_small_large_small_in_one_process():
    """A launch below the 64 KiB limit, one that opts in to more, then the first again: the same exact planes."""
    small = _strip_masks(np.random.default_rng(1), 5, 8190)
    tiny = _strip_masks(np.random.default_rng(2), 37, 53)
    first = _check_strip(small)
    _check_strip(tiny)
    _check_strip(_strip_masks(np.random.default_rng(3), 5, 16384))
    again = _check_strip(small)
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    _check_strip(tiny)
    _check_strip(_strip_masks(np.random.default_rng(4), 16, 8191))
    _check_strip(small)


# ---- end to end -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw,size", [((45, 61), None), ((270, 480), (60, 34)), ((54, 96), (96, 108))],
                         ids=["same", "down", "one_axis"])
def test_interpolate_masks_equals_the_composed_arbiters(hw, size):
    pytest.importorskip("PIL.Image")
    pytest.importorskip("scipy.ndimage")
    h, w = hw
    rng = np.random.default_rng(h + w)
    indices, count = [2, 7, 11, 12], 15
    keys = np.stack([_blob(rng, h, w) for _ in indices])
    out = videomask.interpolate_masks({i: k for i, k in zip(indices, keys)}, count, size=size, device=DEV)
    got = out.cpu().numpy()
    centroids = []
    for k in keys:
        ys, xs = np.nonzero(k >= 0.5)
        centroids.append((int(ys.sum()) / len(ys), int(xs.sum()) / len(xs)) if len(ys) else None)
    assert all(c is not None for c in centroids)
    want = vref.morph_ref(keys, frame_plan(indices, count, centroids))
    if size is not None:
        want = vref.pil_resize_ref(vref.codes_ref(want), size)
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.abs(got - want).max() <= 1.0 / 255.0 + 1e-7
    assert np.mean(got == want) >= 0.9999
    assert not got[:2].any() and not got[13:].any() and got[3:7].any()
