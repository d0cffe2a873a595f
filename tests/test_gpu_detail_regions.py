"""The per-region Detailer on the MI355X (lanpaint_amd.detail, csrc/label_kernel.hip, csrc/detail_kernel.hip):
lp_mask_components against the numpy labelling of tests/regions_ref.py, lp_detail_resample_regions and lp_detail_stitch_regions
bit for bit against the single-region entries called once per region with CPU-built region masks, the composed stitch against
the torch restatement, and the two nodes.  Every comparison covers every element."""
import copy

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, detail, detail_nodes, detail_region_nodes
from tests import detail_ref, regions_ref
from tests.compare import _tensor_bits as _bits
from tests.device import DEV, _gen

pytestmark = pytest.mark.gpu
CAP = _cabi.LP_DETAIL_MAX_COMPONENTS


# ---- lp_mask_components ------------------------------------------------------------------------------------------------------------
def _check_components(mask, what):
    """mask: CPU tensor, or a HIP tensor to be used as it is (its alignment matters).  Labels (every element), count and table
    (every row below the cap) equal label_ref of the union over planes."""
    labels, n, table = detail.mask_components(mask if mask.is_cuda else mask.to(DEV))
    want_labels, want_n, want_table = regions_ref.label_ref(regions_ref.union_set(mask.cpu().numpy()))
    assert labels.is_cuda and labels.dtype == torch.int32 and tuple(labels.shape) == tuple(mask.shape[-2:])
    assert n == want_n, (what, n, want_n)
    assert np.array_equal(labels.cpu().numpy(), want_labels), what
    assert len(table) == min(n, CAP) and np.array_equal(np.array(table, np.int64).reshape(-1, 5), want_table[:CAP]), what
    return labels, n, table


@pytest.mark.parametrize("shape", [(3, 70, 130), (1, 257, 1000), (2, 33, 77), (1, 16, 64), (5, 300, 1028), (130, 70)])
def test_components_equal_label_ref_on_random_masks(shape):
    g = _gen(shape[-1])
    for density in (0.0005, 0.01, 0.3):
        mask = (torch.rand(shape, generator=g) < density).float() * torch.rand(shape, generator=g)    # soft values, some <= 0.5
        _, n, _ = _check_components(mask, (shape, density))
        print(f"COMPONENTS {shape} density {density}: n = {n}")


def test_components_are_of_the_union_over_frames_and_take_2d_masks():
    mask = torch.zeros(4, 90, 200)
    mask[0, 10:30, 150:170] = 1.0
    mask[2, 29:50, 169:190] = 1.0              # touches frame 0's square at one corner, in another frame: one component
    mask[3, 80, 20] = mask[1, 81, 21] = 1.0    # a diagonal pair split over two frames
    mask[1, 60, 100] = 1.0
    _, n, table = _check_components(mask, "union")
    assert n == 3 and table[0] == (10, 49, 150, 189, 20 * 20 + 21 * 21 - 1)
    assert _check_components(mask[2], "2-D")[1] == 1
    assert _check_components(mask[:, :, 3:], "strided view")[1] == 3


def _serpentine(H, W):
    S = np.zeros((H, W), bool)
    S[0::2, :] = True
    for i, y in enumerate(range(1, H, 2)):
        S[y, W - 1 if i % 2 == 0 else 0] = True
    return S


def _spiral(H, W):
    S = np.zeros((H, W), bool)
    top, left, bottom, right = 0, 0, H - 1, W - 1
    S[0, :] = True
    while bottom - top >= 4 and right - left >= 4:                      # walls two apart, one pixel wide, one long path
        S[top:bottom + 1, right] = True
        S[bottom, left:right + 1] = True
        S[top + 2:bottom + 1, left] = True
        S[top + 2, left:right - 1] = True
        top, left, bottom, right = top + 2, left + 2, bottom - 2, right - 2
    return S


def test_components_long_chains_and_diagonals():
    H, W = 500, 1300
    for name, S in (("serpentine", _serpentine(H, W)), ("spiral", _spiral(H, W))):
        _, n, table = _check_components(torch.from_numpy(S).float().unsqueeze(0), name)
        assert n == 1 and table[0][:4] == (0, H - 1, 0, W - 1), (name, n)
    checker = torch.from_numpy(np.indices((H, W)).sum(0) % 2 == 0).float()       # diagonal-only: one component, not H * W / 2
    _, n, table = _check_components(checker, "checkerboard")
    assert n == 1 and table[0] == (0, H - 1, 0, W - 1, H * W // 2)
    anti = torch.zeros(70, 70)
    anti[torch.arange(70), 69 - torch.arange(70)] = 1.0                          # NE / SW neighbours only, across tile corners
    assert _check_components(anti, "anti-diagonal")[1] == 1


@pytest.mark.parametrize("H,W", [(64, 256), (37, 101), (1, 1), (500, 1300)])
def test_components_full_empty_corners_and_the_threshold(H, W):
    for planes in (1, 3):
        _, n, table = _check_components(torch.ones(planes, H, W), "full")
        assert n == 1 and table == ((0, H - 1, 0, W - 1, H * W),)
        labels, n, table = _check_components(torch.zeros(planes, H, W), "empty")
        assert n == 0 and table == () and int(labels.abs().max()) == 0
        corners = torch.zeros(planes, H, W)
        for y, x in {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)}:
            corners[planes - 1, y, x] = 1.0
        assert _check_components(corners, "corners")[1] == (1 if (H, W) == (1, 1) else 4)
        soft = torch.full((planes, H, W), 0.5)                         # 0.5 itself is not set; the next float above it is
        assert _check_components(soft, "0.5")[1] == 0
        soft[planes - 1, H // 3, W // 4] = float(np.nextafter(np.float32(0.5), np.float32(0)))
        soft[0, H // 2, W // 2] = float(np.nextafter(np.float32(0.5), np.float32(1)))
        _, n, table = _check_components(soft, "nextafter")
        assert n == 1 and table == ((H // 2, H // 2, W // 2, W // 2, 1),)
    with pytest.raises(ValueError, match="empty"):
        detail.plan_regions(detail.mask_components(torch.zeros(1, H, W, device=DEV)), H, W)


@pytest.mark.parametrize("shape", [(2, 64, 128), (1, 33, 77), (3, 50, 66)])
def test_components_on_a_mask_that_does_not_start_on_16_bytes(shape):
    """The 16-bytes-per-lane union pass needs H * W % 4 == 0 and an aligned base; everything else takes the scalar pass."""
    mask = (torch.rand(shape, generator=_gen(shape[1])) < 0.2).float()
    n_el = mask.numel()
    for offset in (0, 1, 2):
        buf = torch.zeros(n_el + 4, device=DEV)
        view = buf[offset:offset + n_el].view(shape)
        view.copy_(mask)
        assert view.is_contiguous() and view.data_ptr() % 16 == (4 * offset) % 16
        _check_components(view, (shape, offset))


def test_components_past_the_cap_keep_labels_and_count_exact_and_plan_one_region():
    H, W = 257, 1000
    mask = (torch.rand(1, H, W, generator=_gen(7)) < 0.3).float()
    labels, n, table = _check_components(mask, "overflow")             # labels exact, table[0] the true count, 4096 rows exact
    print(f"COMPONENTS overflow: n = {n}")
    assert n > CAP and len(table) == CAP
    bbox = detail.mask_bbox(mask.to(DEV))
    r = detail.plan_regions((n, table), H, W, 1.5, 8, 8, 0, 64, 8, bbox=bbox)
    assert len(r) == 1 and r.region(0) == detail.plan_region(bbox, H, W, 1.5, 8, 8, 0) and r.members == (tuple(range(1, n + 1)),)
    image = torch.rand(1, H, W, 3, generator=_gen(8))
    cimg, cmask = detail.crop_regions(image.to(DEV), mask.to(DEV), r, labels, "bilinear")       # every label is a member
    want_img, want_mask = detail.crop_resample(image.to(DEV), mask.to(DEV), r.region(0), "bilinear")
    assert np.array_equal(_bits(cimg), _bits(want_img)) and np.array_equal(_bits(cmask), _bits(want_mask))
    cimg2, cmask2, st, count = detail_region_nodes.LanPaint_DetailerCropRegions().crop(image, mask, 1.5, 8, 0, 8, "bilinear", 64, 8)
    assert count == 1 and np.array_equal(_bits(cimg2), _bits(want_img)) and np.array_equal(_bits(cmask2), _bits(want_mask))


# ---- scenes for crop and stitch ------------------------------------------------------------------------------------------------
# blobs as (frame, y0, y1, x0, x1), inclusive.  Inside a blob the mask is soft above 0.5, outside it is soft at or below 0.3
# (label 0: kept in every region's mask).
SEPARATE = (150, 220, [(0, 20, 50, 30, 70), (0, 90, 130, 150, 200), (0, 100, 120, 20, 45), (0, 14, 16, 74, 77)])
OVERLAP = (160, 240, [(0, 20, 99, 40, 55), (0, 60, 75, 70, 149), (0, 120, 140, 200, 220)])   # equalised windows of 1 and 2 overlap


def _scene(scene, b, mask_b, c, seed):
    H, W, blobs = scene
    mask = torch.zeros(mask_b, H, W)
    for i, (_, y0, y1, x0, x1) in enumerate(blobs):
        mask[i % mask_b, y0:y1 + 1, x0:x1 + 1] = 1.0
    noise = torch.rand(mask.shape, generator=_gen(seed))
    mask = torch.where(mask > 0, 0.55 + 0.45 * noise, 0.3 * noise * (noise > 0.8))
    image = torch.rand(b, H, W, c, generator=_gen(seed + 1))
    return image, mask


def _plan(mask, H, W, target, min_area=1, max_regions=8, context=1.0, padding=0):
    labels, n, table = _check_components(mask, "scene")
    regions = detail.plan_regions((n, table), H, W, context, padding, 8, target, min_area, max_regions)
    ref_labels = regions_ref.label_ref(regions_ref.union_set(mask.numpy()))[0]
    masks = [regions_ref.region_mask(mask, ref_labels, mem) for mem in regions.members]      # on the CPU, from label_ref
    return labels, regions, masks, ref_labels


@pytest.mark.parametrize("target", [0, 96])
@pytest.mark.parametrize("filter", detail.FILTERS)
@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("b", [1, 3])
def test_crop_regions_is_crop_resample_per_region_bit_for_bit(b, c, filter, target):
    H, W, _ = SEPARATE
    for mask_b in sorted({1, b}):
        image, mask = _scene(SEPARATE, b, mask_b, c, 10 * b + c)
        labels, regions, masks, _ = _plan(mask, H, W, target, min_area=20)
        assert len(regions) == 3 and regions.resampled == (target > 0)        # the 3 x 4 blob is below min_area: nobody's
        cimg, cmask = detail.crop_regions(image.to(DEV), mask.to(DEV), regions, labels, filter)
        assert tuple(cimg.shape) == (3 * b, regions.oh, regions.ow, c) and tuple(cmask.shape) == (3 * mask_b, regions.oh, regions.ow)
        erased = 0
        for i in range(3):
            want_img, want_mask = detail.crop_resample(image.to(DEV), masks[i].to(DEV), regions.region(i), filter)
            assert np.array_equal(_bits(cimg[i * b:(i + 1) * b]), _bits(want_img)), (i, "image")
            assert np.array_equal(_bits(cmask[i * mask_b:(i + 1) * mask_b]), _bits(want_mask)), (i, "mask")
            erased += int((masks[i] != mask).sum())
        assert erased > 0
        only_img, none = detail.crop_regions(image.to(DEV), None, regions, None, filter)
        assert none is None and np.array_equal(_bits(only_img), _bits(cimg))


def test_crop_regions_erases_foreign_components_inside_a_window():
    """Windows that hold pixels of another region's component: those pixels read 0, soft background values stay."""
    H, W, _ = OVERLAP
    image, mask = _scene(OVERLAP, 2, 2, 3, 5)
    labels, regions, masks, ref_labels = _plan(mask, H, W, 0)
    assert len(regions) == 3 and int(regions_ref.cover_count(regions).max()) == 2
    _, cmask = detail.crop_regions(image.to(DEV), mask.to(DEV), regions, labels)
    cmask = cmask.cpu()
    foreign_seen = 0
    for i, (y0, x0) in enumerate(regions.origins):
        window = (slice(None), slice(y0, y0 + regions.h), slice(x0, x0 + regions.w))
        assert torch.equal(cmask[2 * i:2 * i + 2], masks[i][window])
        lab = torch.from_numpy(ref_labels)[window[1:]]
        foreign = (lab != 0) & (lab != regions.members[i][0])
        foreign_seen += int(foreign.sum())
        assert bool((cmask[2 * i:2 * i + 2][:, foreign] == 0).all())
        assert torch.equal(cmask[2 * i:2 * i + 2][:, lab == 0], mask[window][:, lab == 0])
    assert foreign_seen > 0


def _compose_parent(original, det, masks, regions, k, filter):
    b = original.shape[0]
    out = original.to(DEV)
    for i in range(len(regions)):
        out = detail.stitch(out, det[i * b:(i + 1) * b].to(DEV), masks[i].to(DEV), regions.region(i), k, filter)
    return out


def _outside_windows_untouched(out, original, regions):
    outside = torch.from_numpy(regions_ref.cover_count(regions) == 0)
    return bool(outside.any()) and torch.equal(out[:, outside], original[:, outside])


@pytest.mark.parametrize("target", [0, 104])
@pytest.mark.parametrize("filter", detail.FILTERS)
@pytest.mark.parametrize("k", [1, 9, 51])
@pytest.mark.parametrize("scene,b,mask_b,c", [(SEPARATE, 2, 1, 3), (OVERLAP, 1, 1, 4), (OVERLAP, 3, 3, 3)],
                         ids=["separate", "overlap", "overlap_mask_per_frame"])
def test_stitch_regions_is_the_composition_of_stitch_and_meets_the_torch_restatement(scene, b, mask_b, c, k, filter, target):
    H, W, _ = scene
    image, mask = _scene(scene, b, mask_b, c, 40 + k)
    labels, regions, masks, ref_labels = _plan(mask, H, W, target, min_area=20)
    cover = int(regions_ref.cover_count(regions).max())
    assert len(regions) == 3 and regions.resampled == (target > 0) and cover == (2 if scene is OVERLAP else 1)
    det = torch.rand(3 * b, regions.oh, regions.ow, c, generator=_gen(50 + k))
    out = detail.stitch_regions(image.to(DEV), det.to(DEV), mask.to(DEV), regions, labels, k, filter)
    assert out.is_cuda and out.dtype == torch.float32
    want = _compose_parent(image, det, masks, regions, k, filter)
    assert np.array_equal(_bits(out), _bits(want))                                # bit for bit, every element
    out = out.cpu()
    assert _outside_windows_untouched(out, image, regions)
    ref = regions_ref.stitch_regions_ref(image, det, mask, regions, ref_labels, k, filter)
    bnd = detail_ref.bound((regions.oh, regions.ow), (regions.h, regions.w), filter, float(det.abs().max()))
    err = float((out - ref).abs().max())
    print(f"STITCH_REGIONS k={k} {filter} target={target} cover={cover}: max err {err:.3g}, atol {cover * (3e-6 + bnd):.3g}")
    assert err <= cover * (3e-6 + bnd)


def test_stitch_regions_without_labels_uses_the_mask_as_it_is():
    H, W, _ = SEPARATE
    image, mask = _scene(SEPARATE, 2, 1, 3, 3)
    labels, regions, _, _ = _plan(mask, H, W, 0)
    det = torch.rand(len(regions) * 2, regions.oh, regions.ow, 3, generator=_gen(4))
    out = detail.stitch_regions(image.to(DEV), det.to(DEV), mask.to(DEV), regions, None, 9)
    want = _compose_parent(image, det, [mask] * len(regions), regions, 9, "bilinear")
    assert np.array_equal(_bits(out), _bits(want))


# ---- nodes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filter", detail.FILTERS)
@pytest.mark.parametrize("target", [0, 256])
def test_region_nodes_with_one_region_equal_the_existing_nodes_bit_for_bit(target, filter):
    H, W = 150, 200
    image = torch.rand(3, H, W, 3, generator=_gen(31))
    mask = torch.zeros(3, H, W)
    mask[0, 30:61, 50:91] = 1.0
    mask[2, 100:131, 140:181] = 1.0                                     # two blobs, apart
    noise = torch.rand(mask.shape, generator=_gen(8))
    mask = torch.where(mask > 0, 0.55 + 0.45 * noise, 0.3 * noise * (noise > 0.8))
    old_img, old_mask, old_st = detail_nodes.LanPaint_DetailerCrop().crop(image, mask, 1.25, 4, target, 8, filter)
    cimg, cmask, st, count = detail_region_nodes.LanPaint_DetailerCropRegions().crop(image, mask, 1.25, 4, target, 8, filter, 1, 1)
    assert count == 1 and st["regions"].region(0) == old_st["region"] and st["regions"].members == ((1, 2),)
    assert cimg.device.type == "cpu" and cmask.device.type == "cpu"
    assert np.array_equal(_bits(cimg), _bits(old_img)) and np.array_equal(_bits(cmask), _bits(old_mask))
    inpainted = (cimg * 0.5 + 0.25).contiguous()
    old_out, = detail_nodes.LanPaint_DetailerStitch().stitch(old_st, inpainted, 9)
    out, = detail_region_nodes.LanPaint_DetailerStitchRegions().stitch(copy.deepcopy(st), inpainted, 9)
    assert out.device.type == "cpu" and np.array_equal(_bits(out), _bits(old_out))
    two = detail_region_nodes.LanPaint_DetailerCropRegions().crop(image, mask, 1.25, 4, target, 8, filter, 1, 8)
    assert two[3] == 2 and two[0].shape[0] == 6 and two[1].shape[0] == 6


@pytest.mark.parametrize("k", [1, 9])
def test_region_nodes_round_trip_identity_inpaint_with_three_regions(k):
    H, W = 160, 256
    image = torch.rand(2, H, W, 3, generator=_gen(21))
    mask = torch.zeros(1, H, W)
    for y0, y1, x0, x1 in [(16, 40, 24, 56), (100, 130, 30, 70), (60, 90, 180, 220)]:
        mask[0, y0:y1 + 1, x0:x1 + 1] = 1.0
    cimg, cmask, st, count = detail_region_nodes.LanPaint_DetailerCropRegions().crop(image, mask, 1.0, 8, 0, 8, "bicubic", 64, 8)
    regions = st["regions"]
    assert count == 3 and int(regions_ref.cover_count(regions).max()) == 1 and tuple(cimg.shape) == (6, regions.h, regions.w, 3)
    for i, (y0, x0) in enumerate(regions.origins):
        assert torch.equal(cimg[2 * i:2 * i + 2], image[:, y0:y0 + regions.h, x0:x0 + regions.w, :])
        assert torch.equal(cmask[i:i + 1], mask[:, y0:y0 + regions.h, x0:x0 + regions.w])      # nothing foreign in a window
    out, = detail_region_nodes.LanPaint_DetailerStitchRegions().stitch(copy.deepcopy(st), cimg, k)
    assert out.device.type == "cpu" and _outside_windows_untouched(out, image, regions)
    assert bool(((out - image).abs() <= 5 * 2.0 ** -24 * image.abs()).all())
