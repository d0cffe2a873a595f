"""Detailer crop / stitch, the parts that need no device: the region plan's hand-computed known answers, the antialias tap
tables against torch's fp64 operator, the nodes' protocol, and the C ABI's argument checks (made before any HIP call)."""
import ctypes

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, detail
from tests import detail_ref

SHAPES = [((300, 417), (1024, 1424)), ((1024, 1424), (300, 417)), ((731, 512), (736, 512)), ((97, 55), (41, 200)),
          ((64, 48), (64, 48))]


# ---- region plan: every expected value below is worked out by hand from the rule in detail.py's docstring -------------------
def _r(*v):
    return detail.Region(*v)


def test_plan_mask_in_a_corner():
    # rows 0..49, columns 0..99 of 512 x 768; context 1.0, padding 0, M = 8, target 0
    # y: n = 50, need = 56, e = 6, lo = 0 - 3 -> shifted back to 0.   x: n = 100, need = 104, e = 4, lo = -2 -> 0
    assert detail.plan_region((0, 49, 0, 99), 512, 768, 1.0, 0, 8, 0) == _r(0, 0, 56, 104, 56, 104, 512, 768)
    # context 1.5, padding 32, target 1024:  y: g = 32 + ceil(500 * 50 / 2000) = 45, [0, 95), need 96, e = 1, lo stays 0
    # x: g = 32 + 25 = 57, [0, 157), need 160, e = 3, lo = -1 -> 0.   L = 160: oh = floor((2*96*1024 + 1280) / 2560) = 77 -> 616
    # (614.4 / 8 = 76.8), ow = floor((2*160*1024 + 1280) / 2560) = 128 -> 1024
    assert detail.plan_region((0, 49, 0, 99), 512, 768, 1.5, 32, 8, 1024) == _r(0, 0, 96, 160, 616, 1024, 512, 768)


def test_plan_mask_touching_two_borders():
    # rows 400..511, columns 700..767 of 512 x 768 (bottom right); context 1.5, padding 0, M = 16, target 0
    # y: side 112, g = ceil(500 * 112 / 2000) = 28, [372, 512), n = 140, need 144, e = 4, lo = 370 -> shifted to 512 - 144 = 368
    # x: side 68, g = 17, [683, 768), n = 85, need 96, e = 11, lo = 683 - 5 = 678 -> shifted to 768 - 96 = 672
    assert detail.plan_region((400, 511, 700, 767), 512, 768, 1.5, 0, 16, 0) == _r(368, 672, 144, 96, 144, 96, 512, 768)


def test_plan_interior_multiple_of_8_and_16_target_0_and_1024():
    # rows 100..229 (130), columns 301..420 (120) of 600 x 800; context 1.0, padding 0
    # M = 8:  y: need 136, e = 6, lo = 97.   x: need 120, e = 0
    assert detail.plan_region((100, 229, 301, 420), 600, 800, 1.0, 0, 8, 0) == _r(97, 301, 136, 120, 136, 120, 600, 800)
    # M = 16: y: need 144, e = 14, lo = 93.  x: need 128, e = 8, lo = 297.  target 1024, L = 144:
    # oh = floor((2*144*1024 + 2304) / 4608) = 64 -> 1024;  ow = floor((2*128*1024 + 2304) / 4608) = floor(57.39) = 57 -> 912
    assert detail.plan_region((100, 229, 301, 420), 600, 800, 1.0, 0, 16, 1024) == _r(93, 297, 144, 128, 1024, 912, 600, 800)


def test_plan_context_counts_in_thousandths():
    # context 1.1 is 1100 thousandths whatever its binary fraction: side 100, g = ceil(100 * 100 / 2000) = 5 exactly
    # [445, 555), n = 110, need 112, e = 2, lo = 444
    assert detail.plan_region((450, 549, 450, 549), 1000, 1000, 1.1, 0, 8, 0) == _r(444, 444, 112, 112, 112, 112, 1000, 1000)


def test_plan_without_room_for_a_multiple():
    # 5 x 6 image, M = 8: need 8 > 5 and 8 > 6, the region stays as grown
    assert detail.plan_region((1, 2, 2, 4), 5, 6, 1.0, 0, 8, 0) == _r(1, 2, 2, 3, 2, 3, 5, 6)
    # target 1024, L = 3: oh = floor((2*2*1024 + 24) / 48) = 85 -> 680, ow = floor((2*3*1024 + 24) / 48) = 128 -> 1024
    assert detail.plan_region((1, 2, 2, 4), 5, 6, 1.0, 0, 8, 1024) == _r(1, 2, 2, 3, 680, 1024, 5, 6)
    # 100 x 100, rows / columns 10..89, padding 32: clamped to [0, 100), need 104 > 100: stays 100, not a multiple
    assert detail.plan_region((10, 89, 10, 89), 100, 100, 1.0, 32, 8, 0) == _r(0, 0, 100, 100, 100, 100, 100, 100)


def test_plan_rejects_an_empty_mask_and_bad_arguments():
    with pytest.raises(ValueError, match="empty"):
        detail.plan_region((64, -1, 48, -1), 64, 48)                # what lp_mask_bbox returns for an empty mask
    for kw in ({"context": 0.9}, {"padding": -1}, {"multiple_of": 0}, {"target": -8}):
        with pytest.raises(ValueError):
            detail.plan_region((1, 2, 3, 4), 64, 48, **kw)
    with pytest.raises(ValueError):
        detail.plan_region((1, 64, 3, 4), 64, 48)


# ---- tap tables ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filter", detail.FILTERS)
@pytest.mark.parametrize("in_hw,out_hw", SHAPES + detail_ref.ALL_PAIRS)
def test_aa_coeffs_are_torchs_antialias_rule(in_hw, out_hw, filter):
    x = torch.rand(1, in_hw[0], in_hw[1], 1, dtype=torch.float64, generator=torch.Generator().manual_seed(in_hw[0] + out_hw[1]))
    want = detail_ref.torch_aa(x.movedim(-1, 1), out_hw, filter)[0, 0].numpy()       # F.interpolate; see there for a width of 1
    got = detail_ref.apply_tables64(x[0, :, :, 0].numpy(), out_hw, filter)
    err = float(np.abs(got - want).max())
    print(f"{in_hw}->{out_hw} {filter}: max |tables - F.interpolate| = {err:.3g}")
    assert got.shape == want.shape and err <= 1e-12
    for size_in, size_out in zip(in_hw, out_hw):
        bounds, weights = detail.aa_coeffs(size_in, size_out, filter)
        assert bounds.dtype == np.int32 and weights.dtype == np.float64 and weights.shape[0] == size_out
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds.sum(1) <= size_in).all()
        assert bounds[:, 1].max() <= weights.shape[1]
        np.testing.assert_allclose(weights.sum(1), 1.0, atol=1e-14)
        if size_in == size_out:                 # the identity table: weight 1 on the tap itself, exact zeros beside it
            assert np.array_equal(detail_ref.dense(bounds, weights, size_in), np.eye(size_in))


@pytest.mark.parametrize("filter", detail.FILTERS)
@pytest.mark.parametrize("in_hw,out_hw", SHAPES[:4] + detail_ref.ALL_PAIRS)
def test_fp32_restatement_of_the_kernel_is_inside_the_derived_bound(in_hw, out_hw, filter):
    """The GPU test holds lp_detail_resample to detail_ref.bound; here numpy fp32 sums stand in for the kernel."""
    x = torch.rand(in_hw, dtype=torch.float32, generator=torch.Generator().manual_seed(7))
    want = detail_ref.ref64(x[None, :, :, None], out_hw, filter)[0, :, :, 0].numpy()
    err = float(np.abs(detail_ref.apply_tables32(x.numpy(), out_hw, filter).astype(np.float64) - want).max())
    b = detail_ref.bound(in_hw, out_hw, filter, float(x.abs().max()))
    print(f"{in_hw}->{out_hw} {filter}: e = {err:.3g}, b = {b:.3g}")
    assert err <= b


@pytest.mark.parametrize("filter", detail.FILTERS)
@pytest.mark.parametrize("in_hw,out_hw", detail_ref.ALL_PAIRS)
def test_fp32_restatement_equals_the_impulse_reference_exactly(in_hw, out_hw, filter):
    """tests/test_gpu_detail_shapes.py holds lp_detail_resample to detail_ref.impulse_ref as values, exactly; here the numpy
    restatement of the kernel, which sums every tap in order, is held to it at the same sites."""
    sites = detail_ref.impulse_sites(in_hw, out_hw, filter)
    assert len(sites) >= 1 and all(0 <= sy < in_hw[0] and 0 <= sx < in_hw[1] for sy, sx in sites)
    if (in_hw, out_hw) == ((2000, 40), (50, 40)):
        assert len(sites) == 9                  # the first and the last of its four tiles span more than one chunk
    for sy, sx in sites:
        x = np.zeros(in_hw, np.float32)
        x[sy, sx] = detail_ref.IMPULSE
        want = detail_ref.impulse_ref(in_hw, out_hw, filter, (sy, sx))
        got = detail_ref.apply_tables32(x, out_hw, filter)
        assert got.dtype == np.float32 and want.shape == tuple(out_hw) and np.array_equal(got, want), (sy, sx)
        assert np.count_nonzero(want) > 0       # every source element reaches some output


def test_aa_coeffs_rejects_bad_arguments():
    with pytest.raises(ValueError):
        detail.aa_coeffs(8, 8, "lanczos")
    with pytest.raises(ValueError):
        detail.aa_coeffs(0, 8)


# ---- Python API: no CPU fallback ------------------------------------------------------------------------------------------------
def test_detail_refuses_cpu_tensors():
    img, mask = torch.zeros(1, 16, 16, 3), torch.zeros(1, 16, 16)
    region = detail.plan_region((2, 5, 2, 5), 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        detail.mask_bbox(mask)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        detail.crop_resample(img, mask, region)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        detail.stitch(img, img[:, :8, :8], mask, region, 3)
    with pytest.raises(ValueError):
        detail.stitch(img, img, mask, region, 4)
    with pytest.raises(ValueError):
        detail.crop_resample(img, mask, region, "nearest")


# ---- nodes ----------------------------------------------------------------------------------------------------------------------
def test_node_protocol_and_own_mappings():
    from lanpaint_amd import detail_nodes, nodes
    crop, stitch = detail_nodes.LanPaint_DetailerCrop, detail_nodes.LanPaint_DetailerStitch
    assert detail_nodes.NODE_CLASS_MAPPINGS == {"LanPaint_DetailerCrop": crop, "LanPaint_DetailerStitch": stitch}
    assert set(detail_nodes.NODE_DISPLAY_NAME_MAPPINGS) == set(detail_nodes.NODE_CLASS_MAPPINGS)
    assert not set(detail_nodes.NODE_CLASS_MAPPINGS) & set(nodes.NODE_CLASS_MAPPINGS)
    req = crop.INPUT_TYPES()["required"]
    assert list(req) == ["image", "mask", "context", "padding", "target", "multiple_of", "filter"]
    assert req["image"][0] == "IMAGE" and req["mask"][0] == "MASK" and req["context"][0] == "FLOAT"
    assert req["context"][1]["min"] == 1.0 and req["padding"][1]["min"] == 0 and req["target"][1]["min"] == 0
    assert req["multiple_of"][1]["default"] == 8 and req["filter"][0] == ["bilinear", "bicubic"]
    assert crop.RETURN_TYPES == ("IMAGE", "MASK", "LANPAINT_STITCH") and crop.FUNCTION == "crop"
    req = stitch.INPUT_TYPES()["required"]
    assert list(req) == ["stitch", "image", "blend_overlap"] and req["stitch"][0] == "LANPAINT_STITCH"
    assert req["blend_overlap"][1] == {**req["blend_overlap"][1], "min": 1, "max": 51, "step": 2}
    assert stitch.RETURN_TYPES == ("IMAGE",) and stitch.FUNCTION == "stitch"
    for cls in (crop, stitch):
        assert callable(getattr(cls, cls.FUNCTION)) and cls.CATEGORY == "image"


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
def test_detail_entries_reject_bad_arguments_without_a_device(hip_lib):
    C, E, U = ctypes, _cabi.LP_E_INVALID, _cabi.LP_E_UNSUPPORTED
    p = C.c_void_p(256)                                    # never dereferenced: validation comes before any HIP call
    for args in ((None, 1, 8, 8, p), (p, 1, 8, 8, None), (p, 0, 8, 8, p), (p, 1, 0, 8, p), (p, 1, 8, -2, p),
                 (p, 1, _cabi.LP_DETAIL_MAX_SIDE + 1, 8, p)):
        assert hip_lib.lp_mask_bbox(*args, None) == E, args
    assert hip_lib.lp_mask_bbox(p, 65536, 8, 8, p, None) == U

    assert hip_lib.lp_detail_resample(None, None) == E
    good = dict(batch=2, src_h=32, src_w=40, channels=3, y0=4, x0=8, win_h=16, win_w=24, out_h=32, out_w=48, ksize_x=3,
                ksize_y=3, src=p, bounds_x=p, weights_x=p, bounds_y=p, weights_y=p, dst=p)
    for change in ({"batch": 0}, {"src_h": 0}, {"channels": 0}, {"channels": 65}, {"win_h": 0}, {"win_w": -1}, {"y0": -1},
                   {"x0": 17}, {"y0": 17}, {"win_w": 33}, {"out_h": 0}, {"out_w": _cabi.LP_DETAIL_MAX_SIDE + 1},
                   {"ksize_x": 0}, {"ksize_y": -1}, {"src": None}, {"dst": None}, {"bounds_x": None}, {"weights_y": None}):
        d = _cabi.LpDetailResampleDesc(**{**good, **change})
        assert hip_lib.lp_detail_resample(C.byref(d), None) == E, change
    assert hip_lib.lp_detail_resample(C.byref(_cabi.LpDetailResampleDesc(**{**good, "dst": 260})), None) == _cabi.LP_E_ALIGN
    assert hip_lib.lp_detail_resample(C.byref(_cabi.LpDetailResampleDesc(**{**good, "batch": 65536})), None) == U

    assert hip_lib.lp_detail_stitch(None, None) == E
    good = dict(batch=2, height=32, width=40, channels=3, y0=4, x0=8, win_h=16, win_w=24, k=9, mask_batch=1, mask=p,
                original=p, detail=p, out=C.c_void_p(512))
    for change in ({"batch": 0}, {"height": 0}, {"width": _cabi.LP_DETAIL_MAX_SIDE + 1}, {"channels": 0}, {"win_h": 0},
                   {"x0": -1}, {"x0": 17}, {"win_h": 29}, {"k": 0}, {"k": 8}, {"k": 53}, {"mask_batch": 3}, {"mask": None},
                   {"original": None}, {"detail": None}, {"out": None}, {"out": p}):
        d = _cabi.LpDetailStitchDesc(**{**good, **change})
        assert hip_lib.lp_detail_stitch(C.byref(d), None) == E, change
    assert hip_lib.lp_detail_stitch(C.byref(_cabi.LpDetailStitchDesc(**{**good, "batch": 65536, "mask_batch": 1})), None) == U
