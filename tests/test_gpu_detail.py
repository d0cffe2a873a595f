"""The Detailer's HIP kernels on the MI355X (lanpaint_amd.detail, csrc/detail_kernel.hip): lp_mask_bbox against torch.nonzero,
lp_detail_resample against torch's fp64 antialiased interpolate under a bound derived from the tap tables, lp_detail_stitch
against a torch CPU restatement and against lp_mask_blend, and the two nodes on CPU tensors.  Every comparison covers every
output element."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lanpaint_amd import blend, detail, detail_nodes
from tests import detail_ref
from tests.device import DEV, _gen
from tests.image_checks import _bbox_ref, _outside_is_untouched, _rect_mask, _region
from tests.image_inputs import STITCH_CASES

pytestmark = pytest.mark.gpu
SHAPES = [((300, 417), (1024, 1424)), ((1024, 1424), (300, 417)), ((731, 512), (736, 512)), ((97, 55), (41, 200))]


# ---- lp_mask_bbox ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 70, 130), (1, 257, 1000), (2, 33, 77), (1, 16, 64), (5, 300, 1028), (130, 70)])
def test_bbox_equals_torch_nonzero_on_random_sparse_masks(shape):
    g = _gen(shape[-1])
    for density in (0.0005, 0.01, 0.3):
        mask = (torch.rand(shape, generator=g) < density).float() * torch.rand(shape, generator=g)    # soft values, some <= 0.5
        assert detail.mask_bbox(mask.to(DEV)) == _bbox_ref(mask), (shape, density)


@pytest.mark.parametrize("H,W", [(64, 256), (37, 101), (1, 1), (500, 1300)])
def test_bbox_single_pixels_soft_values_and_empty(H, W):
    for planes in (1, 3):
        for y, x in {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 3)}:
            mask = torch.zeros(planes, H, W)
            mask[planes - 1, y, x] = 1.0
            assert detail.mask_bbox(mask.to(DEV)) == (y, y, x, x)
        empty = torch.zeros(planes, H, W)
        assert detail.mask_bbox(empty.to(DEV)) == (H, -1, W, -1)
        soft = torch.full((planes, H, W), 0.5)                         # 0.5 itself is not set; the next float above it is
        assert detail.mask_bbox(soft.to(DEV)) == (H, -1, W, -1)
        soft[planes - 1, H // 3, W // 4] = float(np.nextafter(np.float32(0.5), np.float32(0)))
        soft[0, H // 2, W // 2] = float(np.nextafter(np.float32(0.5), np.float32(1)))
        assert detail.mask_bbox(soft.to(DEV)) == (H // 2, H // 2, W // 2, W // 2) == _bbox_ref(soft)
    with pytest.raises(ValueError, match="empty"):
        detail.plan_region(detail.mask_bbox(torch.zeros(1, H, W, device=DEV)), H, W)


def test_bbox_is_the_union_over_frames_and_takes_2d_masks():
    mask = torch.zeros(4, 90, 200)
    mask[0, 10, 150] = mask[2, 80, 20] = mask[3, 40, 199] = 1.0
    assert detail.mask_bbox(mask.to(DEV)) == (10, 80, 20, 199)
    assert detail.mask_bbox(mask[2].to(DEV)) == (80, 80, 20, 20)
    assert detail.mask_bbox(mask[:, :, 3:].to(DEV)) == (10, 80, 17, 196)       # a strided view: made contiguous, scalar path


# ---- lp_detail_resample ----------------------------------------------------------------------------------------------------------
def _check_resample(image, region, filter, label):
    """image [B, H, W, C] on the CPU.  e_hip <= b over every output element; e_t32 (torch's own fp32 CPU operator) for the record."""
    r = region
    crop = image[:, r.y0:r.y0 + r.h, r.x0:r.x0 + r.w, :].contiguous()
    want = detail_ref.ref64(crop, (r.oh, r.ow), filter)
    got, _ = detail.crop_resample(image.to(DEV), None, r, filter)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape)
    e_hip = float((got.cpu().double() - want).abs().max())
    b = detail_ref.bound((r.h, r.w), (r.oh, r.ow), filter, float(crop.abs().max()))
    t32 = F.interpolate(crop.movedim(-1, 1), size=(r.oh, r.ow), mode=filter, align_corners=False, antialias=True).movedim(1, -1)
    e_t32 = float((t32.double() - want).abs().max())
    print(f"DETAIL_ACC {label} {filter} B={image.shape[0]} C={image.shape[3]} ({r.h},{r.w})->({r.oh},{r.ow}): "
          f"e_hip={e_hip:.3g} b={b:.3g} e_t32={e_t32:.3g}")
    assert e_hip <= b


@pytest.mark.parametrize("filter", detail.FILTERS)
@pytest.mark.parametrize("case", range(4))
def test_resample_window_inside_a_larger_image_meets_the_derived_bound(case, filter):
    in_hw, out_hw = SHAPES[case]
    b, c = [(3, 3), (1, 4), (3, 1), (1, 3)][case] if filter == "bilinear" else [(1, 4), (3, 1), (1, 3), (3, 4)][case]
    y0, x0 = 37 + case, 53 - case
    H, W = in_hw[0] + y0 + 29, in_hw[1] + x0 + 18
    image = torch.rand(b, H, W, c, generator=_gen(100 + case))
    _check_resample(image, _region(y0, x0, in_hw, out_hw, H, W), filter, "window")


@pytest.mark.parametrize("filter", detail.FILTERS)
@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("b", [1, 3])
def test_resample_every_channel_and_batch_count_flush_with_each_border(b, c, filter):
    H, W = 120, 80
    image = torch.rand(b, H, W, c, generator=_gen(b * 10 + c))
    for y0, x0, hw, out_hw in [(0, 12, (97, 55), (41, 200)), (23, 14, (97, 55), (41, 200)), (11, 0, (97, 55), (200, 41)),
                               (9, 25, (97, 55), (41, 200)), (0, 0, (120, 80), (250, 33)), (23, 25, (97, 55), (97, 200))]:
        _check_resample(image, _region(y0, x0, hw, out_hw, H, W), filter, "border")


@pytest.mark.parametrize("c", [1, 3, 4])
def test_resample_same_size_is_a_bitwise_copy(c):
    image = torch.randn(3, 75, 133, c, generator=_gen(c))
    image[0, 20, 30, 0] = -0.0
    for y0, x0, h, w in [(0, 0, 75, 133), (5, 9, 64, 101), (74, 132, 1, 1)]:
        for filter in detail.FILTERS:
            got, _ = detail.crop_resample(image.to(DEV), None, _region(y0, x0, (h, w), (h, w), 75, 133), filter)
            want = image[:, y0:y0 + h, x0:x0 + w, :].contiguous()
            assert np.array_equal(got.cpu().numpy().view(np.uint32), want.numpy().view(np.uint32))


@pytest.mark.parametrize("mask_b", [1, 3])
def test_mask_is_cropped_by_the_same_job_bilinear_and_stays_soft(mask_b):
    H, W = 140, 210
    image = torch.rand(3, H, W, 3, generator=_gen(5))
    mask = torch.rand(mask_b, H, W, generator=_gen(6))
    r = _region(16, 40, (96, 128), (160, 216), H, W)
    _, got = detail.crop_resample(image.to(DEV), mask.to(DEV), r, "bicubic")
    want = detail_ref.ref64(mask[:, 16:112, 40:168, None], (160, 216), "bilinear")[..., 0]
    assert tuple(got.shape) == (mask_b, 160, 216)
    e = float((got.cpu().double() - want).abs().max())
    assert e <= detail_ref.bound((96, 128), (160, 216), "bilinear", float(mask.max()))
    assert float(((got > 0.02) & (got < 0.98)).float().mean()) > 0.9          # soft: not binarised


# ---- lp_detail_stitch ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 9, 51])
@pytest.mark.parametrize("case", STITCH_CASES, ids=[c[0] for c in STITCH_CASES])
def test_stitch_without_resample_matches_torch_restatement_and_mask_blend(case, k):
    name, b, H, W, c, mb, rects, soft, context, padding = case
    original = torch.rand(b, H, W, c, generator=_gen(1))
    mask = _rect_mask((mb, H, W), rects, soft)
    region = detail.plan_region(detail.mask_bbox(mask.to(DEV)), H, W, context, padding, 8, 0)
    assert not region.resampled
    det = torch.rand(b, region.oh, region.ow, c, generator=_gen(2))
    out = detail.stitch(original.to(DEV), det.to(DEV), mask.to(DEV), region, k, "bilinear")
    assert out.is_cuda
    out = out.cpu()
    want = detail_ref.stitch_ref(original, det, mask, region, k, "bilinear")
    err = float((out - want).abs().max())
    print(f"DETAIL_STITCH {name} k={k}: region {region}, max err {err:.3g}")
    assert err <= 3e-6
    assert _outside_is_untouched(out, original, region)
    # the old kernel over the whole frame agrees inside the region
    r = region
    pasted = original.clone()
    pasted[:, r.y0:r.y0 + r.h, r.x0:r.x0 + r.w, :] = det
    old = blend.mask_blend(original.to(DEV), pasted.to(DEV), mask.to(DEV), k).cpu()
    inside = (slice(None), slice(r.y0, r.y0 + r.h), slice(r.x0, r.x0 + r.w))
    assert float((out[inside] - old[inside]).abs().max()) <= 3e-6


@pytest.mark.parametrize("filter", detail.FILTERS)
@pytest.mark.parametrize("k", [1, 9, 51])
@pytest.mark.parametrize("case", STITCH_CASES, ids=[c[0] for c in STITCH_CASES])
def test_stitch_with_resample_back_matches_torch_restatement(case, k, filter):
    name, b, H, W, c, mb, rects, soft, context, padding = case
    original = torch.rand(b, H, W, c, generator=_gen(11))
    mask = _rect_mask((mb, H, W), rects, soft)
    region = detail.plan_region(detail.mask_bbox(mask.to(DEV)), H, W, context, padding, 8, 104)
    assert region.resampled
    det = torch.rand(b, region.oh, region.ow, c, generator=_gen(12))
    out = detail.stitch(original.to(DEV), det.to(DEV), mask.to(DEV), region, k, filter).cpu()
    want = detail_ref.stitch_ref(original, det, mask, region, k, filter)
    bnd = detail_ref.bound((region.oh, region.ow), (region.h, region.w), filter, float(det.abs().max()))
    err = float((out - want).abs().max())
    print(f"DETAIL_STITCH {name} k={k} {filter}: region {region}, max err {err:.3g}, atol {3e-6 + bnd:.3g}")
    assert err <= 3e-6 + bnd
    assert _outside_is_untouched(out, original, region)


# ---- nodes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 9])
def test_node_round_trip_identity_inpaint_without_resample(k):
    H, W = 128, 160
    image = torch.rand(2, H, W, 3, generator=_gen(21))
    mask = _rect_mask((1, H, W), [(0, 40, 70, 60, 110)])
    cimg, cmask, st = detail_nodes.LanPaint_DetailerCrop().crop(image, mask, 1.5, 8, 0, 8, "bicubic")
    r = st["region"]
    assert cimg.device.type == "cpu" and cmask.device.type == "cpu" and tuple(cimg.shape) == (2, r.h, r.w, 3)
    assert torch.equal(cimg, image[:, r.y0:r.y0 + r.h, r.x0:r.x0 + r.w, :])
    assert torch.equal(cmask, mask[:, r.y0:r.y0 + r.h, r.x0:r.x0 + r.w])
    out, = detail_nodes.LanPaint_DetailerStitch().stitch(copy.deepcopy(st), cimg, k)
    assert out.device.type == "cpu" and _outside_is_untouched(out, image, r)
    # m as the kernels compute it (lp_mask_blend's smooth_out runs the same tile passes)
    _, m = blend._launch(mask.to(DEV), image.to(DEV), image.to(DEV), k, want_smooth=True)
    m = m.cpu().expand(2, H, W).unsqueeze(-1).expand_as(image)
    exact = (m == 0) | (m == 1)
    assert torch.equal(out[exact], image[exact])
    assert bool(((out - image).abs() <= 5 * 2.0 ** -24 * image.abs()).all())
    if k > 1:
        assert bool((~exact).any())


@pytest.mark.parametrize("filter", detail.FILTERS)
def test_node_with_resample_equals_the_python_api_bit_for_bit(filter):
    H, W = 150, 200
    image = torch.rand(3, H, W, 3, generator=_gen(31))
    mask = _rect_mask((3, H, W), [(0, 30, 60, 50, 90), (2, 45, 80, 70, 120)], soft_seed=8)
    cimg, cmask, st = detail_nodes.LanPaint_DetailerCrop().crop(image, mask, 1.25, 4, 256, 8, filter)
    r = st["region"]
    assert r == detail.plan_region(detail.mask_bbox(mask.to(DEV)), H, W, 1.25, 4, 8, 256) and r.resampled
    want_img, want_mask = detail.crop_resample(image.to(DEV), mask.to(DEV), r, filter)
    assert cimg.device.type == "cpu" and torch.equal(cimg, want_img.cpu())
    assert cmask.device.type == "cpu" and torch.equal(cmask, want_mask.cpu())
    inpainted = (cimg * 0.5 + 0.25).contiguous()
    st2 = copy.deepcopy(st)
    assert st2["region"] == r and torch.equal(st2["original"], image) and torch.equal(st2["mask"], mask)
    out, = detail_nodes.LanPaint_DetailerStitch().stitch(st2, inpainted, 9)
    want = detail.stitch(image.to(DEV), inpainted.to(DEV), mask.to(DEV), r, 9, filter)
    assert out.device.type == "cpu" and torch.equal(out, want.cpu())
    assert _outside_is_untouched(out, image, r)
