"""The Detailer's HIP kernels on the MI355X at the shapes where kernels go wrong (csrc/detail_kernel.hip, resample_tile.h,
mask_tile.h, label_kernel.hip), each against a live reference that shares nothing with them: lp_detail_resample against
torch's fp64 operator under the derived bound and, for images with one non-zero element, against the tap tables exactly;
lp_detail_stitch against the torch restatement on images smaller than its halo, at the tile switch, on strips at the side
limit; the boxes against numpy; the labellings against scipy.  Every comparison covers every output element."""
import ctypes

import numpy as np
import pytest
import torch
from scipy import ndimage

from lanpaint_amd import _cabi, detail, detail_subjects
from lanpaint_amd._util import raw_stream
from tests import detail_ref, regions_ref, subjects_ref
from tests.compare import _tensor_bits as _bits
from tests.device import DEV, _gen
from tests.image_checks import _rect_mask, _region
from tests.image_inputs import STITCH_CASES

pytestmark = pytest.mark.gpu
CAP = _cabi.LP_DETAIL_MAX_COMPONENTS
SIDE = _cabi.LP_DETAIL_MAX_SIDE
Y0, X0, AFTER_Y, AFTER_X = 3, 5, 2, 3               # every window: at an odd origin of a larger image, rows and columns after it


# ---- lp_detail_resample ----------------------------------------------------------------------------------------------------------
def _around(window):
    """window [B, h, w, C] inside an image whose other elements are 100 and more: a read outside the window shows."""
    b, h, w, c = window.shape
    image = 100.0 + torch.rand(b, h + Y0 + AFTER_Y, w + X0 + AFTER_X, c, generator=_gen(h + w))
    image[:, Y0:Y0 + h, X0:X0 + w, :] = window
    return image


def _chunks(in_h, out_h, filter):
    return max(-(-(yhi - ylo) // 32) for ylo, yhi in detail_ref.tile_rows(in_h, out_h, filter))


def _check_impulses(in_hw, out_hw, c, filter):
    """One image of the batch per non-zero element, one launch: the sites of detail_ref.impulse_sites in channel 0, the centre
    in the last channel, and the pixel just outside each edge of the window, whose response is all zeros.  Equal as values to
    detail_ref.impulse_ref, every element.  Returns the number of images compared."""
    (h, w), (oh, ow) = in_hw, out_hw
    H, W = h + Y0 + AFTER_Y, w + X0 + AFTER_X
    inside = [(sy, sx, 0) for sy, sx in detail_ref.impulse_sites(in_hw, out_hw, filter)] + [(h // 2, w // 2, c - 1), (h - 1, 0, c - 1)]
    inside = list(dict.fromkeys(inside))
    outside = [(-1, w // 2), (h, w // 2), (h // 2, -1), (h // 2, w), (-1, -1), (h, w)]
    image = torch.zeros(len(inside) + len(outside), H, W, c)
    want = np.zeros((image.shape[0], oh, ow, c), np.float32)
    for i, (sy, sx, ch) in enumerate(inside):
        image[i, Y0 + sy, X0 + sx, ch] = detail_ref.IMPULSE
        want[i, :, :, ch] = detail_ref.impulse_ref(in_hw, out_hw, filter, (sy, sx))
    for i, (sy, sx) in enumerate(outside, len(inside)):
        image[i, Y0 + sy, X0 + sx, c - 1] = detail_ref.IMPULSE
    got, _ = detail.crop_resample(image.to(DEV), None, _region(Y0, X0, in_hw, out_hw, H, W), filter)
    got = got.cpu().numpy()
    assert got.shape == want.shape
    for i in range(image.shape[0]):
        assert np.array_equal(got[i], want[i]), (in_hw, out_hw, filter, (inside + outside)[i],
                                                 int((got[i] != want[i]).sum()), float(np.abs(got[i] - want[i]).max()))
    return image.shape[0]


def _check_pair(family, in_hw, out_hw, c, filter, batch=1):
    """Random in [0, 1), random in [-1, 1) and a constant 1.0 under detail_ref.bound against torch's fp64 operator, then the
    impulses exactly.  Prints the DETAIL_SHAPES line of the case; its figures are those of the [0, 1) input."""
    (h, w), (oh, ow) = in_hw, out_hw
    g = _gen(h * 7 + ow)
    kinds = {"unit": torch.rand(batch, h, w, c, generator=g), "signed": torch.rand(batch, h, w, c, generator=g) * 2.0 - 1.0,
             "one": torch.ones(batch, h, w, c)}
    figures = {}
    for kind, window in kinds.items():
        image = _around(window)
        want = detail_ref.ref64(window, out_hw, filter)
        got, _ = detail.crop_resample(image.to(DEV), None, _region(Y0, X0, in_hw, out_hw, image.shape[1], image.shape[2]), filter)
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape)
        got = got.cpu().double()
        e_hip = float((got - want).abs().max())
        b = detail_ref.bound(in_hw, out_hw, filter, float(window.abs().max()))
        figures[kind] = (e_hip, b)
        if kind == "unit":
            t32 = detail_ref.torch_aa(window.movedim(-1, 1), out_hw, filter).movedim(1, -1)
            e_t32 = float((t32.double() - want).abs().max())
        if kind == "one":                                          # the weights of a row sum to 1
            assert float((got - 1.0).abs().max()) <= b, (family, in_hw, out_hw, filter)
    impulses = _check_impulses(in_hw, out_hw, c, filter)
    e_hip, b = figures["unit"]
    print(f"DETAIL_SHAPES {family} {filter} B={batch} C={c} ({h},{w})->({oh},{ow}): e_hip={e_hip:.3g} b={b:.3g} e_t32={e_t32:.3g} "
          f"ratio={e_hip / e_t32 if e_t32 else float('nan'):.3g} chunks={_chunks(h, oh, filter)} impulses={impulses} "
          f"e_signed={figures['signed'][0]:.3g} e_one={figures['one'][0]:.3g}")
    for kind, (e, bnd) in figures.items():
        assert e <= bnd, (family, kind, in_hw, out_hw, filter, e, bnd)


_GENERAL = [(family, pair) for family in ("degenerate", "long_taps", "side_limit") for pair in detail_ref.SHAPE_PAIRS[family]]


@pytest.mark.parametrize("filter", detail.FILTERS)
@pytest.mark.parametrize("family,pair", _GENERAL, ids=[f"{p[0][0]}x{p[0][1]}-{p[1][0]}x{p[1][1]}" for _, p in _GENERAL])
def test_resample_degenerate_windows_long_tap_tables_and_sides_at_the_limit(family, pair, filter):
    """1 x 1, 1 x N and N x 1 windows and outputs; 2000 -> 50 and 1100 -> 16 (161 and 277 bicubic taps, up to nine LDS chunks
    a tile), 4096 -> 33 across a row; an output side of LP_DETAIL_MAX_SIDE on either axis."""
    assert SIDE == 32768
    _check_pair(family, pair[0], pair[1], 3, filter)


@pytest.mark.parametrize("filter", detail.FILTERS)
@pytest.mark.parametrize("oh", detail_ref.TILE_OH)
def test_resample_output_rows_around_the_256_element_tile(oh, filter):
    """Output heights 15 / 16 / 17 / 33 by flat row lengths 252 / 255 / 256 / 257 / 260 with one channel and
    252 / 255 / 258 / 261 with three: the 16 B store, the scalar tail and a second block of one lane."""
    for in_hw, out_hw in detail_ref.SHAPE_PAIRS["tile_c1"]:
        if out_hw[0] == oh:
            _check_pair("tile_c1", in_hw, out_hw, 1, filter)
    for in_hw, out_hw in detail_ref.SHAPE_PAIRS["tile_c3"]:
        if out_hw[0] == oh:
            _check_pair("tile_c3", in_hw, out_hw, 3, filter)


@pytest.mark.parametrize("filter", detail.FILTERS)
@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("c", [2, 5, 7, 64])
def test_resample_channel_counts_up_to_the_limit(c, b, filter):
    assert _cabi.LP_DETAIL_MAX_CHANNELS == 64
    for in_hw, out_hw in detail_ref.SHAPE_PAIRS["channels"]:
        _check_pair("channels", in_hw, out_hw, c, filter, batch=b)


@pytest.mark.parametrize("c", [2, 5, 64])
def test_resample_same_size_is_a_bitwise_copy_at_more_channels(c):
    image = torch.randn(2, 23 + Y0 + AFTER_Y, 31 + X0 + AFTER_X, c, generator=_gen(c))
    image[0, Y0, X0, c - 1] = -0.0
    H, W = image.shape[1], image.shape[2]
    for y0, x0, h, w in [(Y0, X0, 23, 31), (0, 0, H, W), (H - 1, W - 1, 1, 1), (1, 1, 1, W - 1), (1, 1, H - 1, 1)]:
        for filter in detail.FILTERS:
            got, _ = detail.crop_resample(image.to(DEV), None, _region(y0, x0, (h, w), (h, w), H, W), filter)
            assert np.array_equal(_bits(got), _bits(image[:, y0:y0 + h, x0:x0 + w, :]))


@pytest.mark.parametrize("filter", detail.FILTERS)
def test_regions_track_and_subjects_forms_at_nine_chunks_and_five_channels(filter):
    """The other window policies instantiate the same kernel: each window bit for bit what crop_resample gives for it."""
    (h, w), (oh, ow) = (2000, 40), (50, 40)
    assert _chunks(h, oh, filter) > 3
    b, c, H, W = 2, 5, h + 9, w + 13
    image = torch.rand(b, H, W, c, generator=_gen(71)).to(DEV)
    mask = torch.rand(b, H, W, generator=_gen(72)).to(DEV)

    def same(got, origins, images):
        got_img, got_mask = got
        assert tuple(got_img.shape) == (len(origins), oh, ow, c) and tuple(got_mask.shape) == (len(origins), oh, ow)
        for i, ((y0, x0), f) in enumerate(zip(origins, images)):
            want_img, want_mask = detail.crop_resample(image[f:f + 1], mask[f:f + 1], _region(y0, x0, (h, w), (oh, ow), H, W), filter)
            assert np.array_equal(_bits(got_img[i]), _bits(want_img[0])), (i, "image")
            assert np.array_equal(_bits(got_mask[i]), _bits(want_mask[0])), (i, "mask")

    regions = detail.Regions(H, W, h, w, oh, ow, ((1, 3), (9, 13)), ((1,), (2,)))
    same(detail.crop_regions(image, mask, regions, None, filter), [(1, 3), (1, 3), (9, 13), (9, 13)], [0, 1, 0, 1])
    track = detail.Track(H, W, h, w, oh, ow, ((7, 1), (3, 11)))
    same(detail.crop_track(image, mask, track, filter), track.origins, [0, 1])
    sub = detail_subjects.Subjects(H, W, h, w, oh, ow, ((1, 1), (5, 7), (9, 13), (3, 5)), 2, ((1,), (2,)))
    same(detail_subjects.crop_subjects(image, mask, sub, None, filter), sub.origins, [0, 1, 0, 1])


@pytest.mark.parametrize("filter", detail.FILTERS)
def test_one_process_many_tables_a_repeated_geometry_is_bitwise_the_same(filter):
    """device_tables caches the uploaded tap tables by geometry: a pair met again after others gives the same bits."""
    first = {}
    order = [((2000, 40), (50, 40)), ((1, 1), (7, 9)), ((40, 4096), (40, 33)), ((2000, 40), (50, 40)), ((1, 1), (7, 9)),
             ((37, 41), (17, 257)), ((40, 4096), (40, 33)), ((2000, 40), (50, 40))]
    for in_hw, out_hw in order:
        image = _around(torch.rand(1, in_hw[0], in_hw[1], 3, generator=_gen(in_hw[0])))
        got, _ = detail.crop_resample(image.to(DEV), None, _region(Y0, X0, in_hw, out_hw, image.shape[1], image.shape[2]), filter)
        bits = _bits(got)
        if (in_hw, out_hw) in first:
            assert np.array_equal(bits, first[in_hw, out_hw]), (in_hw, out_hw)
        else:
            first[in_hw, out_hw] = bits
            want = detail_ref.ref64(image[:, Y0:Y0 + in_hw[0], X0:X0 + in_hw[1], :], out_hw, filter)
            assert float((got.cpu().double() - want).abs().max()) <= detail_ref.bound(in_hw, out_hw, filter, 1.0)


# ---- lp_detail_stitch ------------------------------------------------------------------------------------------------------------
def _check_stitch(original, det, mask, region, k, filter, what):
    """Values in [0, 1): 3e-6 against the torch restatement without a resample back, 3e-6 + bound with one; outside the window
    the original bit for bit."""
    out = detail.stitch(original.to(DEV), det.to(DEV), mask.to(DEV), region, k, filter)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == tuple(original.shape)
    out = out.cpu()
    want = detail_ref.stitch_ref(original, det, mask, region, k, filter)
    tol = 3e-6
    if region.resampled:
        tol += detail_ref.bound((region.oh, region.ow), (region.h, region.w), filter, float(det.abs().max()))
    err = float((out - want).abs().max())
    assert err <= tol, (what, region, k, err, tol)
    r = region
    probe = out.clone()
    probe[:, r.y0:r.y0 + r.h, r.x0:r.x0 + r.w, :] = original[:, r.y0:r.y0 + r.h, r.x0:r.x0 + r.w, :]
    assert np.array_equal(_bits(probe), _bits(original)), (what, region, k)
    return err


@pytest.mark.parametrize("k", [1, 3, 15, 17, 51])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 40), (40, 1), (5, 7), (8, 32), (9, 33), (16, 64), (17, 65)])
def test_stitch_on_images_at_and_below_the_halo(H, W, k):
    """Images smaller than a tile and than the 2R halo on each of its sides: the whole image as the window, without and with
    a resample back, and a 1 x 1 window at each corner.  Soft masks on both sides of 0.5; one plane for two images once."""
    g = _gen(H * 100 + W + k)
    original = torch.rand(2, H, W, 3, generator=g)
    mask = torch.rand(2, H, W, generator=g)
    assert (H * W == 1) or (bool((mask > 0.5).any()) and bool((mask < 0.5).any()))
    worst = _check_stitch(original, torch.rand(2, H, W, 3, generator=g), mask, _region(0, 0, (H, W), (H, W), H, W), k, "bilinear", "whole")
    for filter in detail.FILTERS:
        oh, ow = H + 3, 2 * W + 1
        worst = max(worst, _check_stitch(original, torch.rand(2, oh, ow, 3, generator=g), mask[:1],
                                         _region(0, 0, (H, W), (oh, ow), H, W), k, filter, "whole, resampled, one mask plane"))
    for y0, x0 in sorted({(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)}) if H * W > 1 else []:
        worst = max(worst, _check_stitch(original, torch.rand(2, 1, 1, 3, generator=g), mask, _region(y0, x0, (1, 1), (1, 1), H, W),
                                         k, "bilinear", "corner"))
    print(f"DETAIL_SHAPES stitch_small {H}x{W} k={k}: max err {worst:.3g}")


@pytest.mark.parametrize("k", [15, 17])
@pytest.mark.parametrize("h,w", [(15, 63), (16, 64), (17, 65), (7, 31), (8, 32), (9, 33)])
def test_stitch_either_side_of_the_tile_switch_on_one_scene(h, w, k):
    """k = 15 is the last width on the 16 x 64 tile, k = 17 the first on the 8 x 32 one: windows one less than, equal to and
    one more than either tile, flush with each corner of a 96 x 128 scene and once inside it."""
    name, b, H, W, c, mb, rects, soft, _, _ = next(case for case in STITCH_CASES if case[0] == "one_mask_for_three_frames")
    assert (H, W) == (96, 128)
    original = torch.rand(b, H, W, c, generator=_gen(k))
    mask = _rect_mask((mb, H, W), rects, soft)
    det = torch.rand(b, h, w, c, generator=_gen(h))
    worst = 0.0
    for y0, x0 in [(0, 0), (0, W - w), (H - h, 0), (H - h, W - w), (37, 45)]:
        worst = max(worst, _check_stitch(original, det, mask, _region(y0, x0, (h, w), (h, w), H, W), k, "bilinear", name))
    print(f"DETAIL_SHAPES stitch_tile_switch {h}x{w} k={k}: max err {worst:.3g}")


@pytest.mark.parametrize("k", [1, 9, 17])
@pytest.mark.parametrize("c", [2, 5, 64])
def test_stitch_channel_counts_up_to_the_limit(c, k):
    H, W = 40, 50
    g = _gen(c * 10 + k)
    original = torch.rand(2, H, W, c, generator=g)
    mask = torch.rand(2, H, W, generator=g)
    worst = _check_stitch(original, torch.rand(2, 24, 33, c, generator=g), mask, _region(5, 7, (24, 33), (24, 33), H, W), k, "bilinear", "same")
    for filter in detail.FILTERS:
        worst = max(worst, _check_stitch(original, torch.rand(2, 36, 45, c, generator=g), mask, _region(5, 7, (24, 33), (36, 45), H, W),
                                         k, filter, "resampled"))
    print(f"DETAIL_SHAPES stitch_channels C={c} k={k}: max err {worst:.3g}")


@pytest.mark.parametrize("H,W,k", [(SIDE, 8, 9), (8, SIDE, 9), (8, SIDE, 51)])
def test_stitch_on_strips_at_the_side_limit(H, W, k):
    """The whole strip as the window, and a 200-long window at its far end.  (The torch restatement of the 32768 x 8 strip at
    k = 51 alone takes two seconds on the CPU: not run.)"""
    g = _gen(H + k)
    original = torch.rand(1, H, W, 3, generator=g)
    mask = torch.rand(1, H, W, generator=g)
    worst = _check_stitch(original, torch.rand(1, H, W, 3, generator=g), mask, _region(0, 0, (H, W), (H, W), H, W), k, "bilinear", "strip")
    h, w = min(H, 200), min(W, 200)
    worst = max(worst, _check_stitch(original, torch.rand(1, h, w, 3, generator=g), mask, _region(H - h, W - w, (h, w), (h, w), H, W),
                                     k, "bilinear", "far end"))
    print(f"DETAIL_SHAPES stitch_strip {H}x{W} k={k}: max err {worst:.3g}")


def _small_scene():
    """9 x 33, two frames: a blob on the left, one on the right, a small one between them that no window owns.  Soft inside
    (above 0.5) and outside (at or below 0.3)."""
    H, W = 9, 33
    S = torch.zeros(2, H, W, dtype=torch.bool)
    S[:, 2:6, 3:9] = True
    S[:, 1:8, 20:29] = True
    S[:, 7:9, 13:15] = True
    noise = torch.rand(S.shape, generator=_gen(17))
    return H, W, S, torch.where(S, 0.55 + 0.45 * noise, 0.3 * noise)


def test_stitch_regions_track_and_subjects_on_an_image_below_the_halo():
    """k = 17 on 9 x 33: each form bit for bit the single-window stitch, window after window, with the mask erased in torch."""
    H, W, S, mask = _small_scene()
    k, b, c, h, w = 17, 2, 3, 9, 16
    original = torch.rand(b, H, W, c, generator=_gen(1))
    # regions: labels of the union over frames, by scipy
    lab2, n = ndimage.label(S.any(0).numpy(), np.ones((3, 3), np.int32))
    assert n == 3
    left, right = int(lab2[2, 3]), int(lab2[1, 20])
    regions = detail.Regions(H, W, h, w, h, w, ((0, 0), (0, 17)), ((left,), (right,)))
    labels = torch.from_numpy(lab2.astype(np.int32)).to(DEV)
    det = torch.rand(2 * b, h, w, c, generator=_gen(2))
    out = detail.stitch_regions(original.to(DEV), det.to(DEV), mask.to(DEV), regions, labels, k)
    want = original.to(DEV)
    for i in range(2):
        erased = regions_ref.region_mask(mask, lab2, regions.members[i])
        assert bool((erased != mask).any())
        want = detail.stitch(want, det[i * b:(i + 1) * b].to(DEV), erased.to(DEV), regions.region(i), k)
    assert np.array_equal(_bits(out), _bits(want))
    # track: frame f's window at its own origin
    track = detail.Track(H, W, 5, 12, 5, 12, ((0, 0), (4, 21)))
    det = torch.rand(b, 5, 12, c, generator=_gen(3))
    out = detail.stitch_track(original.to(DEV), det.to(DEV), mask.to(DEV), track, k)
    for f in range(b):
        want = detail.stitch(original[f:f + 1].to(DEV), det[f:f + 1].to(DEV), mask[f:f + 1].to(DEV), track.region(f), k)
        assert np.array_equal(_bits(out[f]), _bits(want[0])), f
    # subjects: labels of the volume, by scipy
    lab3, n, _ = subjects_ref.label_frames_ref(S.numpy())
    assert n == 3
    members = ((int(lab3[0, 2, 3]),), (int(lab3[0, 1, 20]),))
    sub = detail_subjects.Subjects(H, W, h, w, h, w, ((0, 0), (0, 1), (0, 17), (0, 16)), 2, members)
    det = torch.rand(2 * b, h, w, c, generator=_gen(4))
    out = detail_subjects.stitch_subjects(original.to(DEV), det.to(DEV), mask.to(DEV), sub, torch.from_numpy(lab3).to(DEV), k)
    want = original.to(DEV).clone()
    for s in range(2):
        erased = subjects_ref.subject_mask(mask, lab3, members[s]).to(DEV)
        for f in range(b):
            i = s * b + f
            want[f:f + 1] = detail.stitch(want[f:f + 1].contiguous(), det[i:i + 1].to(DEV), erased[f:f + 1], sub.window(s, f), k)
    assert np.array_equal(_bits(out), _bits(want))


# ---- lp_mask_bbox, lp_mask_bbox_frames ---------------------------------------------------------------------------------------------
def _boxes_numpy(mask):
    """mask numpy [planes, H, W] -> (the box of the union, a box per plane), np.nonzero per plane; (H, -1, W, -1) when empty."""
    planes, H, W = mask.shape
    per = []
    for p in range(planes):
        ys, xs = np.nonzero(mask[p] > np.float32(0.5))
        per.append((int(ys.min()), int(ys.max()), int(xs.min()), int(xs.max())) if ys.size else (H, -1, W, -1))
    union = (min(b[0] for b in per), max(b[1] for b in per), min(b[2] for b in per), max(b[3] for b in per))
    return union, tuple(per)


def _edge_columns(W):
    """The first and last column of every 1024-column block, and the first and last lane's columns of every wave of the last
    block, for the 16 B form (a block is 1024 columns, a wave 256) and the scalar form (256 and 64)."""
    cols = {0, W - 1}
    for x in range(0, W, 1024):
        cols |= {x, min(x + 1023, W - 1)}
    for block, wave in ((1024, 256), (256, 64)):
        base = (W - 1) // block * block
        for x in range(base, W, wave):
            cols |= {x, min(x + 3, W - 1), min(x + wave - 4, W - 1), min(x + wave - 1, W - 1)}
    return sorted(cols)


@pytest.mark.parametrize("shape", [(1, 1, SIDE), (1, SIDE, 1), (3, 3, SIDE - 1), (2, 16, SIDE)] +
                         [(2, 33, W) for W in (1020, 1024, 1028, 2048, 2052, 4100)])
def test_boxes_of_single_pixels_at_block_and_wave_edges_random_and_empty_masks(shape):
    planes, H, W = shape
    host = np.zeros(shape, np.float32)
    dev = torch.zeros(shape, device=DEV)
    assert detail.mask_bbox(dev) == (H, -1, W, -1) and detail.mask_bbox_frames(dev) == ((H, -1, W, -1),) * planes
    sites = [(i % planes, (i * 7) % H, x) for i, x in enumerate(_edge_columns(W))]
    sites += [(planes - 1, y, x) for y in (0, H - 1) for x in (0, W - 1)] + [(0, y, W // 2) for y in range(0, H, max(H // 5, 1))]
    for p, y, x in dict.fromkeys(sites):
        host[p, y, x] = 1.0
        dev[p, y, x] = 1.0
        union, per = _boxes_numpy(host)
        assert union == (y, y, x, x)
        assert detail.mask_bbox(dev) == union, (shape, p, y, x)
        assert detail.mask_bbox_frames(dev) == per, (shape, p, y, x)
        host[p, y, x] = 0.0
        dev[p, y, x] = 0.0
    g = _gen(W + H)
    for seed in range(2):
        mask = ((torch.rand(shape, generator=g) < 0.001).float() * (0.4 + 0.6 * torch.rand(shape, generator=g)))
        union, per = _boxes_numpy(mask.numpy())
        assert detail.mask_bbox(mask.to(DEV)) == union and detail.mask_bbox_frames(mask.to(DEV)) == per, (shape, seed)
    print(f"DETAIL_SHAPES boxes {shape}: {len(dict.fromkeys(sites))} single pixels, 2 random masks, the empty mask")


# ---- lp_subject_boxes ----------------------------------------------------------------------------------------------------------------
def _raw_subject_boxes(labels, owner, subjects, guard=64):
    frames, H, W = labels.shape
    table = torch.full((subjects * frames * 4 + guard,), -7, dtype=torch.int32, device=DEV)
    lab, own = torch.from_numpy(labels).to(DEV), torch.from_numpy(owner).to(DEV)
    assert _cabi.load().lp_subject_boxes(lab.data_ptr(), frames, H, W, own.data_ptr(), own.numel(), subjects, table.data_ptr(),
                                         raw_stream(DEV)) == _cabi.LP_OK
    host = table.cpu().numpy()
    assert bool((host[subjects * frames * 4:] == -7).all())
    return host[:subjects * frames * 4].reshape(subjects, frames, 4).astype(np.int64)


@pytest.mark.parametrize("H", [15, 16, 17, 33])
@pytest.mark.parametrize("W", [256, 257, 300, 1000])
def test_subject_boxes_on_label_volumes_built_by_hand(W, H):
    """Every per-lane branch of lp_detail_subject_boxes_kernel past the first block of columns, by design and not by a
    labelling's chance: a second subject in every lane's column, no uniform wave, every wave uniform with a subject of its
    own, and labels and owner values that are nobody's."""
    F = 3
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")

    def volume(plane):
        v = np.repeat(plane[None].astype(np.int32), F, 0)
        v[1] = 0                                                   # frame 0 whole, frame 1 empty, frame 2 cut on three sides
        v[2, :2, :] = 0
        v[2, :, :11] = 0
        v[2, :, W - 6:] = 0
        return v

    cases = {"rows_alternate": (volume(1 + yy % 2), ((1,), (2,))),
             "columns_alternate": (volume(1 + xx % 3), ((1,), (2,), (3,))),
             "stripes": (volume(1 + xx // 64), tuple((s + 1,) for s in range((W + 63) // 64)))}
    plane = 1 + xx % 3
    plane[(yy + xx) % 5 == 0] = 4                                   # owner_len itself
    plane[(yy + xx) % 5 == 1] = 1 << 20                             # far past it
    plane[(yy + xx) % 5 == 2] = -3
    nobody = volume(plane)
    nobody[0, H - 1, W - 1] = np.iinfo(np.int32).max
    cases["labels_past_the_table"] = (nobody, ((1,), (2,), (3,)))
    for name, (labels, members) in cases.items():
        want = subjects_ref.subject_boxes_ref(labels, members)
        got = detail_subjects.subject_boxes(torch.from_numpy(labels).to(DEV), members)
        assert np.array_equal(np.array(got, np.int64), want), (name, H, W)
        assert all(tuple(want[s, 1]) == (H, -1, W, -1) for s in range(len(members)))
    # the raw entry: owner values 0 and subjects + 1 are nobody's; guard words after the box table
    labels = volume(1 + (xx + yy) % 6)
    owner = np.array([2, 1, 0, 2, 3, 1, 2], np.int32)               # owner[0] is never read; label 2 -> 0, label 4 -> subjects + 1
    members = ((1, 5), (3, 6))
    got = _raw_subject_boxes(labels, owner, 2)
    assert np.array_equal(got, subjects_ref.subject_boxes_ref(labels, members)), (H, W)


# ---- lp_mask_components, lp_mask_components_frames ---------------------------------------------------------------------------------
def _scipy_plane(S):
    labels, n, table = subjects_ref.label_frames_ref(np.asarray(S, bool)[None])      # one frame: 26-connected is 8-connected
    return labels[0], n, table[:, 2:]


def _check_plane(S, what):
    mask = torch.from_numpy(np.asarray(S, bool)).float()
    labels, n, table = detail.mask_components(mask.to(DEV))
    want_labels, want_n, want_table = _scipy_plane(S)
    assert n == want_n, (what, n, want_n)
    assert np.array_equal(labels.cpu().numpy(), want_labels), what
    assert len(table) == min(n, CAP) and np.array_equal(np.array(table, np.int64).reshape(-1, 5), want_table[:CAP]), what
    return n, table


def _check_volume(S, what):
    mask = torch.from_numpy(np.asarray(S, bool)).float()
    labels, n, table = detail_subjects.mask_components_frames(mask.to(DEV))
    want_labels, want_n, want_table = subjects_ref.label_frames_ref(S)
    assert n == want_n, (what, n, want_n)
    assert np.array_equal(labels.cpu().numpy(), want_labels), what
    assert len(table) == min(n, CAP) and np.array_equal(np.array(table, np.int64).reshape(-1, 7), want_table[:CAP]), what
    return n, table


def _strip_masks(shape, seed):
    full = np.ones(shape, bool)
    second = np.zeros(shape, bool)
    second.reshape(-1)[::2] = True
    rand = (torch.rand(shape, generator=_gen(seed)) < 0.4).numpy()
    far = np.zeros(shape, bool)
    far.reshape(-1)[-1] = True
    return {"full": full, "every second": second, "random 0.4": rand, "far end": far}


@pytest.mark.parametrize("H,W", [(1, SIDE), (SIDE, 1), (2, SIDE), (SIDE, 3)])
def test_components_on_strips_at_the_side_limit(H, W):
    """A one-pixel-wide chain across 512 tiles, and H on the border launch's grid."""
    for name, S in _strip_masks((H, W), H + W).items():
        n, table = _check_plane(S, (name, H, W))
        if name == "full":
            assert n == 1 and table == ((0, H - 1, 0, W - 1, H * W),)
        if name == "far end":
            assert n == 1 and table == ((H - 1, H - 1, W - 1, W - 1, 1),)
        print(f"DETAIL_SHAPES components strip {H}x{W} {name}: n = {n}")


@pytest.mark.parametrize("H,W", [(2, 8192), (8192, 2)])
def test_components_frames_on_strips(H, W):
    F = 3
    for name, S in _strip_masks((F, H, W), H + W).items():
        n, table = _check_volume(S, (name, H, W))
        if name == "full":
            assert n == 1 and table == ((0, F - 1, 0, H - 1, 0, W - 1, F * H * W),)
        print(f"DETAIL_SHAPES components_frames strip {F}x{H}x{W} {name}: n = {n}")


@pytest.mark.parametrize("H", [15, 16, 17, 31, 32, 33])
def test_components_around_the_tile_edges_near_the_percolation_threshold(H):
    """Density 0.4: clusters that wind across many 16 x 64 tiles, where concurrent unions meet.  The volume at every width:
    64 and 128 take the 16 B temporal launch, the others the scalar one."""
    for W in (63, 64, 65, 127, 128, 129):
        for seed in (0, 1):
            g = _gen(1000 * H + 10 * W + seed)
            n2, _ = _check_plane((torch.rand(H, W, generator=g) < 0.4).numpy(), (H, W, seed))
            n3, _ = _check_volume((torch.rand(3, H, W, generator=g) < 0.4).numpy(), (3, H, W, seed))
        print(f"DETAIL_SHAPES components tile edge {H}x{W}: n = {n2}, volume n = {n3}")


@pytest.mark.parametrize("n", [CAP - 1, CAP, CAP + 1])
def test_components_at_the_cap_exactly(n):
    """Isolated pixels on a stride-2 grid, n of them: table[0] = n, min(n, cap) rows and the labels exact, and nothing
    written after the table (guard words), for the plane and for the volume."""
    assert CAP == 4096
    for shape in ((128, 130), (3, 66, 130)):
        S = np.zeros(shape, bool)
        S[(slice(0, None, 2),) * len(shape)] = True
        keep = np.flatnonzero(S.reshape(-1))
        assert keep.size > n
        S.reshape(-1)[keep[n:]] = False
        volume = len(shape) == 3
        row, F, (H, W) = (7, shape[0], shape[1:]) if volume else (5, 1, shape)
        want_labels, want_n, want_table = subjects_ref.label_frames_ref(S) if volume else _scipy_plane(S)
        assert want_n == n
        m = torch.from_numpy(S).float().to(DEV)
        out = torch.empty(shape, dtype=torch.int32, device=DEV)
        guarded = torch.full((1 + row * CAP + row * 64,), -7, dtype=torch.int32, device=DEV)
        ws_bytes = _cabi.lp_components_frames_ws_bytes(F, H, W)
        ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=DEV)
        entry = _cabi.load().lp_mask_components_frames if volume else _cabi.load().lp_mask_components
        assert entry(m.data_ptr(), F, H, W, out.data_ptr(), guarded.data_ptr(), ws.data_ptr(), ws_bytes, raw_stream(DEV)) == _cabi.LP_OK
        host = guarded.cpu().numpy()
        rows = min(n, CAP)
        assert host[0] == n and np.array_equal(host[1:1 + row * rows].reshape(-1, row), want_table[:rows]), shape
        if n < CAP:                                                 # rows the scan reset and nobody filled
            empty = [F, -1, H, -1, W, -1, 0][7 - row:]
            assert np.array_equal(host[1 + row * rows:1 + row * CAP].reshape(-1, row), np.tile(empty, (CAP - rows, 1)))
        assert bool((host[1 + row * CAP:] == -7).all()) and np.array_equal(out.cpu().numpy(), want_labels), shape
        if volume:
            _check_volume(S, shape)
        else:
            _check_plane(S, shape)


# ---- EraseForeign ------------------------------------------------------------------------------------------------------------------
def test_labels_at_past_and_below_the_owner_table_are_nobodys_in_crop_and_stitch():
    """The raw regions entries with a label plane that holds owner_len itself, a label far past it and a negative one: each
    region's result is the single-window entry's on a mask where exactly the foreign and the out-of-table components were
    zeroed in torch, label 0 kept."""
    H, W, b, c, k = 40, 70, 2, 3, 9
    g = _gen(5)
    lab = np.zeros((H, W), np.int32)
    lab[2:12, 3:20] = 1                                             # region 0's
    lab[20:35, 40:66] = 3                                           # region 1's: the table's last entry
    lab[14:18, 5:30] = 2                                            # in the table, nobody's
    lab[5:9, 22:30] = lab[30:38, 32:38] = 4                         # owner_len itself, in both windows
    lab[25:30, 10:25] = lab[17:19, 50:60] = 1 << 24                 # far past it, in both windows
    lab[36:39, 2:12] = lab[36:39, 50:60] = -2
    lab[0, 0] = lab[39, 31] = np.iinfo(np.int32).max
    lab[H - 1, W - 1] = np.iinfo(np.int32).min
    owner_host = np.array([9, 1, 0, 2], np.int32)                   # owner[0] is never read: label 0 is kept before the look-up
    owner_len = owner_host.size
    mask = torch.rand(b, H, W, generator=g)                         # soft, both sides of 0.5, under every label
    image = torch.rand(b, H, W, c, generator=g)
    inside = (lab > 0) & (lab < owner_len)
    owner_of = np.where(inside, owner_host[np.where(inside, lab, 0)], 0)
    erased = [torch.where(torch.from_numpy((lab != 0) & (owner_of != i + 1)), torch.zeros(()), mask) for i in range(2)]
    assert all(bool((e[:, lab == 0] == mask[:, lab == 0]).all()) and bool((e != mask).any()) for e in erased)
    labels, owner = torch.from_numpy(lab).to(DEV), torch.from_numpy(owner_host).to(DEV)
    h, w = 24, 40
    for oh, ow in ((h, w), (36, 56)):                               # the erasing copy; the erasing copy into scratch, then the resample
        regions = detail.Regions(H, W, h, w, oh, ow, ((0, 0), (16, 30)), ((1,), (3,)))
        origins = torch.tensor(regions.origins, dtype=torch.int32, device=DEV)
        got = detail._resample(mask.to(DEV).unsqueeze(-1), regions, "bilinear", origins, labels, owner).squeeze(-1)
        for i in range(2):
            _, want = detail.crop_resample(image.to(DEV), erased[i].to(DEV), regions.region(i), "bilinear")
            assert np.array_equal(_bits(got[i * b:(i + 1) * b]), _bits(want)), (oh, ow, i)
        det = torch.rand(2 * b, oh, ow, c, generator=g).to(DEV)
        small = detail._resample(det, detail.Region(0, 0, oh, ow, h, w, oh, ow), "bilinear") if regions.resampled else det
        orig, m, out = image.to(DEV), mask.to(DEV), torch.empty(b, H, W, c, device=DEV)
        host_origins = (ctypes.c_int32 * 4)(*(v for o in regions.origins for v in o))
        d = _cabi.LpDetailStitchRegionsDesc(b, H, W, c, 2, h, w, k, b, owner_len)
        d.origins = ctypes.cast(host_origins, ctypes.c_void_p)
        d.mask, d.original, d.detail, d.out = m.data_ptr(), orig.data_ptr(), small.data_ptr(), out.data_ptr()
        d.labels, d.owner = labels.data_ptr(), owner.data_ptr()
        assert _cabi.load().lp_detail_stitch_regions(ctypes.byref(d), raw_stream(DEV)) == _cabi.LP_OK
        want = orig
        for i in range(2):
            want = detail.stitch(want, det[i * b:(i + 1) * b], erased[i].to(DEV), regions.region(i), k)
        assert np.array_equal(_bits(out), _bits(want)), (oh, ow)
