"""The Detailer colour match on the MI355X (lanpaint_amd.detail_color, csrc/color_kernel.hip) against the numpy restatement
tests/color_ref.py: lp_color_stats' count exactly and its sums within the worst-case bound of a plain fp64 summation, equal bits
on two calls; lp_color_fit and lp_color_apply bit for bit, fed the device's own tables; and the node end to end, alone and
between the tracked crop and stitch.  Every comparison covers every element."""
import itertools

import numpy as np
import pytest
import torch

from lanpaint_amd import detail_color, detail_color_nodes, detail_track_nodes
from tests import color_ref
from tests.device import DEV
from tests.image_checks import _check_color_stats as _check_stats, _fit_bits
from tests.image_inputs import _blob_mask, _images, _rng

pytestmark = pytest.mark.gpu
TOL = 8 * 2.0 ** -24
ABOVE = np.nextafter(np.float32(0.5), np.float32(1.0))


def _edge_mask(Bm, H, W, seed):
    """Exactly 0.5 everywhere -- kept -- with a few elements at the next float above it -- dropped."""
    rng = _rng(Bm, H, W, seed, 7)
    m = np.full((Bm, H, W), 0.5, dtype=np.float32)
    for p in range(Bm):
        for _ in range(3):
            m[p, rng.integers(H), rng.integers(W)] = ABOVE
    return m


# H, W, C, B, mask_batch, margin.  The tile is 32 x 128: sizes at it, one under, one over, three tiles each way; W % 4 != 0
# takes the element-wise loads, C > 4 the channel groups
STATS_CASES = [(1, 1, 3, 1, 1, 0), (1, 300, 1, 2, 2, 1), (300, 1, 4, 2, 1, 3), (17, 33, 5, 7, 7, 25), (70, 150, 3, 2, 2, 3),
               (32, 128, 4, 2, 1, 1), (31, 127, 3, 1, 1, 25), (33, 129, 1, 7, 1, 0), (70, 300, 3, 2, 2, 25), (70, 300, 5, 1, 1, 3),
               (33, 132, 2, 2, 2, 1), (17, 33, 2, 1, 1, 0), (40, 260, 4, 7, 7, 3), (65, 257, 4, 1, 1, 1)]


@pytest.mark.parametrize("form", ["blob", "edge"])
@pytest.mark.parametrize("case", STATS_CASES, ids=lambda c: "x".join(map(str, c)))
def test_stats_equal_the_restatement(case, form):
    H, W, C, B, Bm, margin = case
    d, r = _images(B, H, W, C, 1)
    mask = (_blob_mask if form == "blob" else _edge_mask)(Bm, H, W, 2)
    _check_stats(d, r, mask, margin, (case, form))
    if form == "blob":
        _check_stats(d, r, None, margin, (case, "no mask"))


def test_stats_further_mask_forms():
    H, W, C, B = 40, 136, 3, 4
    d, r = _images(B, H, W, C, 3)
    every = _check_stats(d, r, None, 8, "no mask").cpu().numpy()
    assert (every[:, 0] == H * W).all()
    zero = _check_stats(d, r, np.zeros((1, H, W), dtype=np.float32), 25, "all zero").cpu().numpy()
    assert (zero.view(np.uint64) == every.view(np.uint64)).all()
    none = _check_stats(d, r, np.ones((B, H, W), dtype=np.float32), 0, "all one").cpu().numpy()
    assert (none == 0.0).all()                                                    # n = 0 and every sum with it
    corners = np.zeros((4, H, W), dtype=np.float32)
    for i, (y, x) in enumerate(((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))):
        corners[i, y, x] = 1.0
    for margin in (0, 3):
        got = _check_stats(d, r, corners, margin, ("corners", margin)).cpu().numpy()
        assert (got[:, 0] == H * W - (margin + 1) ** 2).all()                     # the block is cut at the image's border
    _check_stats(d, r, np.full((1, H, W), np.nan, dtype=np.float32), 0, "nan")     # not <= 0.5: dropped


def test_stats_of_strided_views_and_other_dtypes():
    d, r = _images(3, 24, 70, 4, 4)
    mask = _blob_mask(3, 24, 70, 5)
    dt, rt, mt = (torch.from_numpy(a).to(DEV) for a in (d, r, mask))
    want = detail_color.color_stats(dt[:, ::2, :, :3].contiguous(), rt[:, ::2, :, :3].contiguous(), mt[:, ::2].contiguous(), 2)
    got = detail_color.color_stats(dt[:, ::2, :, :3], rt[:, ::2, :, :3], mt[:, ::2], 2)
    assert torch.equal(got, want)
    ref, _ = color_ref.stats_ref(d[:, ::2, :, :3], r[:, ::2, :, :3], mask[:, ::2], 2)
    assert (got.cpu().numpy()[:, 0] == ref[:, 0]).all()
    half = detail_color.color_stats(dt.double(), rt, mt[0], 2)                     # fp64 image, a [H, W] mask
    assert torch.equal(half, detail_color.color_stats(dt, rt, mt[:1], 2))
    with pytest.raises(ValueError):
        detail_color.color_stats(dt, rt[:, :, :, :3], mt, 2)
    with pytest.raises(ValueError):
        detail_color.color_stats(dt, rt, mt[:2], 2)
    with pytest.raises(ValueError):
        detail_color.color_stats(dt, rt, mt, 26)


# ---- fit ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clip_stats():
    """Eight frames, two clips of four with different drifts, as the device's own stats (fp64, on the device)."""
    B, H, W, C = 8, 40, 72, 3
    rng = _rng(11)
    r = rng.random((B, H, W, C), dtype=np.float32)
    d = np.empty_like(r)
    for i in range(B):
        g0, b0 = (0.8 + 0.03 * i, 0.10 - 0.01 * i) if i < 4 else (1.2 - 0.02 * i, -0.05 + 0.004 * i)
        d[i] = (r[i] * np.float32(g0)).astype(np.float32) + np.float32(b0)
    stats = detail_color.color_stats(torch.from_numpy(d).to(DEV), torch.from_numpy(r).to(DEV),
                                     torch.from_numpy(_blob_mask(B, H, W, 12)).to(DEV), 2)
    return stats


def test_fit_equals_the_restatement_bit_for_bit_over_the_parameter_grid(clip_stats):
    seen = {}
    for method, strength, smooth, clip in itertools.product(("mean_std", "mean"), (0.0, 0.3, 1.0), (0, 1, 3, 9), (0, 4)):
        seen[method, strength, smooth, clip] = _fit_bits(clip_stats, method, strength, smooth, clip)
    for method, smooth in itertools.product(("mean_std", "mean"), (0, 3, 9)):
        one, two = seen[method, 1.0, smooth, 0], seen[method, 1.0, smooth, 4]
        assert (one[3] != two[3]).any() and (one[4] != two[4]).any()             # a window that crossed the clips would show
    for method in ("mean_std", "mean"):
        assert (seen[method, 1.0, 1, 0] == seen[method, 1.0, 1, 4]).all()         # one frame: the clip does not matter
        assert (seen[method, 1.0, 9, 4] == seen[method, 1.0, 0, 4]).all()         # wider than the clip = the whole clip
        assert (seen[method, 1.0, 0, 4][:4] == seen[method, 1.0, 0, 4][0]).all()
        assert (seen[method, 1.0, 3, 4][0] != seen[method, 1.0, 3, 4][1]).any()
    for key, coef in seen.items():
        if key[1] == 0.0:
            assert (coef[..., 0] == 1.0).all() and (coef[..., 1] == 0.0).all(), key   # strength 0: exactly (1, 0)
        if key[0] == "mean":
            assert (coef[..., 0] == 1.0).all(), key
    with pytest.raises(ValueError):
        detail_color.color_fit(clip_stats, "mean_std", 1.0, 1, 3)
    with pytest.raises(ValueError):
        detail_color.color_fit(clip_stats, "mean_std", 1.0, 4, 0)
    with pytest.raises(ValueError):
        detail_color.color_fit(clip_stats.float())


def test_fit_guards():
    # n = 63 fits nothing, n = 64 does: 8 x 16 images, all but 63 / 64 pixels masked
    H, W = 8, 16
    d, r = _images(2, H, W, 3, 21)
    mask = np.ones((2, H * W), dtype=np.float32)
    mask[0, :63], mask[1, :64] = 0.0, 0.0
    stats = _check_stats(d, r, mask.reshape(2, H, W), 0, "count guard")
    assert stats[:, 0].tolist() == [63.0, 64.0]
    coef = _fit_bits(stats, "mean_std", 1.0, 1, 0)
    assert coef[0].tolist() == [[1.0, 0.0]] * 3 and (coef[1, :, 0] != 1.0).all() and (coef[1, :, 1] != 0.0).all()
    pooled = _fit_bits(stats, "mean_std", 1.0, 3, 0)                              # 127 pixels together are enough
    assert (pooled[0] == pooled[1]).all() and (pooled[0, :, 0] != 1.0).all()
    # a flat detail channel keeps gain 1; a reference far wider / far narrower than the detail meets the limits
    rng = _rng(22)
    wide = rng.random((1, 24, 40, 3), dtype=np.float32)
    narrow = (np.float32(0.5) + np.float32(0.001) * (wide - np.float32(0.5))).astype(np.float32)
    narrow[..., 2] = np.float32(0.25)
    up = _fit_bits(_check_stats(narrow, wide, None, 0, "gain up"), "mean_std", 1.0, 1, 0)
    assert up[0, :, 0].tolist() == [4.0, 4.0, 1.0]
    down = _fit_bits(_check_stats(wide, narrow, None, 0, "gain down"), "mean_std", 1.0, 1, 0)
    assert down[0, :2, 0].tolist() == [0.25, 0.25] and down[0, 2, 0] == 0.25          # vr = 0 -> g = 0 -> limited to 0.25
    assert _fit_bits(_check_stats(wide, narrow, None, 0, "gain down"), "mean_std", 0.0, 1, 0).tolist() == [[[1.0, 0.0]] * 3]


# ---- apply ----------------------------------------------------------------------------------------------------------------------------
APPLY_SHAPES = [(1, 1, 1, 1), (2, 17, 33, 3), (3, 8, 16, 3), (2, 4, 4, 5), (2, 64, 100, 3), (7, 5, 7, 4), (1, 70, 150, 4),
                (2, 9, 11, 64)]


@pytest.mark.parametrize("shape", APPLY_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_apply_is_the_unfused_affine_map_bit_for_bit(shape):
    B, H, W, C = shape
    rng = _rng(*shape, 31)
    d = rng.random(shape, dtype=np.float32)
    coef_host = np.stack([rng.uniform(0.25, 4.0, (B, C)), rng.uniform(-0.5, 0.5, (B, C))], axis=-1).astype(np.float32)
    coef = torch.from_numpy(coef_host).to(DEV)
    want = color_ref.apply_ref(d, coef.cpu().numpy())
    fused = (d.astype(np.float64) * coef_host[:, None, None, :, 0] + coef_host[:, None, None, :, 1]).astype(np.float32)
    dt = torch.from_numpy(d).to(DEV)
    got = detail_color.color_apply(dt, coef)
    assert (got.cpu().numpy().view(np.uint32) == want.view(np.uint32)).all()
    if d.size > 1000:
        assert (want != fused).any()                                              # the comparison can tell a fused map apart
    # a base pointer one element past a 16-byte boundary, in and out
    n = d.size
    src = torch.empty(n + 1, dtype=torch.float32, device=DEV)
    src[1:] = dt.reshape(-1)
    dst = torch.empty(n + 1, dtype=torch.float32, device=DEV)
    off = detail_color.color_apply(src[1:].view(shape), coef, out=dst[1:].view(shape))
    assert off.data_ptr() % 16 == 4 and torch.equal(off, got)
    # in place
    work = dt.clone()
    same = detail_color.color_apply(work, coef, out=work)
    assert same.data_ptr() == work.data_ptr() and torch.equal(work, got)
    work = src[1:].view(shape)
    detail_color.color_apply(work, coef, out=work)
    assert torch.equal(work, got)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
DRIFTS = [(0.8, 0.10), (0.9, -0.05), (1.1, 0.02), (1.25, 0.0), (0.95, 0.07)]


def _drift(r):
    """fl(fl(g0 r) + b0) with another (g0, b0) per frame; r a CPU tensor [5, H, W, C]."""
    d = torch.empty_like(r)
    for i, (g0, b0) in enumerate(DRIFTS):
        d[i] = r[i] * np.float32(g0) + np.float32(b0)
    return d


def test_node_recovers_a_per_frame_drift():
    H, W = 70, 150
    r = torch.rand(5, H, W, 3, generator=torch.Generator().manual_seed(41))
    mask = torch.zeros(5, H, W)
    mask[:, 25:45, 50:100] = 1.0
    d = _drift(r)
    assert float((d - r).abs().max()) > 0.1
    node = detail_color_nodes.LanPaint_DetailerColorMatch()
    (out,) = node.match(d, r, mask, "mean_std", 1.0, 8, 1, 0)
    assert out.device == d.device and out.dtype == torch.float32 and tuple(out.shape) == tuple(r.shape)
    err = float((out.double() - r.double()).abs().max())
    print(f"node: max |out - r| = {err / 2.0 ** -24:.3f} x 2^-24")
    assert err <= TOL
    want = color_ref.match_ref(d.numpy(), r.numpy(), mask.numpy(), "mean_std", 1.0, 8, 1, 0)
    assert float(np.abs(out.numpy().astype(np.float64) - want).max()) <= 2.0 ** -22   # the restatement says the same
    (weak,) = node.match(d, r, mask, "mean_std", 0.0, 8, 1, 0)
    assert torch.equal(weak, d)                                                   # strength 0: the input, bit for bit
    (dev_out,) = node.match(d.to(DEV), r.to(DEV), mask.to(DEV), "mean_std", 1.0, 8, 1, 0)
    assert dev_out.is_cuda and torch.equal(dev_out.cpu(), out)


def test_color_match_between_the_tracked_crop_and_stitch():
    F, H, W = 5, 96, 160
    g = torch.Generator().manual_seed(42)
    image = torch.rand(F, H, W, 3, generator=g)
    mask = torch.zeros(F, H, W)
    for f in range(F):
        mask[f, 40:56, 20 + 20 * f: 36 + 20 * f] = 1.0
    crop, stitch = detail_track_nodes.LanPaint_DetailerCropTrack(), detail_track_nodes.LanPaint_DetailerStitchTrack()
    cimg, cmask, st = crop.crop(image, mask, 1.5, 8, 0, 8, "bicubic", 3)
    drifted = _drift(cimg)
    (matched,) = detail_color_nodes.LanPaint_DetailerColorMatch().match(drifted, cimg, cmask, "mean_std", 1.0, 2, 1, 0)
    (want,) = stitch.stitch(st, cimg, 9)
    (got,) = stitch.stitch(st, matched, 9)
    (bad,) = stitch.stitch(st, drifted, 9)
    err = float((got.double() - want.double()).abs().max())
    print(f"track: max |stitched - undrifted| = {err / 2.0 ** -24:.3f} x 2^-24")
    assert err <= TOL and float((bad - want).abs().max()) > 0.05
    track = st["track"]
    outside = torch.ones(F, H, W, dtype=torch.bool)
    for f, (y0, x0) in enumerate(track.origins):
        outside[f, y0:y0 + track.h, x0:x0 + track.w] = False
    assert outside.any() and len(set(track.origins)) > 1
    assert torch.equal(got[outside], image[outside])                              # outside every window: the original's bits
