"""The per-region Detailer, the parts that need no device: the numpy labelling arbiter against scipy, the regions rule's worked
example and properties, the nodes' protocol, and the argument checks of the three C entries (made before any HIP call)."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, detail
from tests import regions_ref


def _random_set(rng, H, W, density):
    return rng.random((H, W)) < density


# ---- the arbiter ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,density", [(70, 130, 0.3), (257, 1000, 0.3), (300, 1028, 0.01), (33, 77, 0.6), (720, 1280, 0.05),
                                         (1, 50, 0.5), (50, 1, 0.5), (16, 64, 0.0), (16, 64, 1.0)])
def test_label_ref_equals_scipy(H, W, density):
    ndimage = pytest.importorskip("scipy.ndimage")
    S = _random_set(np.random.default_rng(H * 1000 + W), H, W, density)
    labels, n, table = regions_ref.label_ref(S)
    want, want_n = ndimage.label(S, structure=np.ones((3, 3)))
    assert n == want_n and labels.dtype == np.int32 and np.array_equal(labels, want)
    objects = ndimage.find_objects(want)
    assert table.shape == (n, 5)
    for i, (sy, sx) in enumerate(objects):
        assert tuple(table[i]) == (sy.start, sy.stop - 1, sx.start, sx.stop - 1, int((want[sy, sx] == i + 1).sum()))


def test_label_ref_known_answers():
    S = np.array([[1, 0, 0, 1, 0],
                  [0, 1, 0, 0, 0],
                  [0, 0, 0, 0, 1],
                  [1, 0, 0, 1, 0]], bool)
    labels, n, table = regions_ref.label_ref(S)
    assert n == 4                                                       # the diagonals join; raster order of first pixels
    assert labels.tolist() == [[1, 0, 0, 2, 0], [0, 1, 0, 0, 0], [0, 0, 0, 0, 3], [4, 0, 0, 3, 0]]
    assert table.tolist() == [[0, 1, 0, 1, 2], [0, 0, 3, 3, 1], [2, 3, 3, 4, 2], [3, 3, 0, 0, 1]]
    checker = np.indices((9, 14)).sum(0) % 2 == 0                       # diagonal-only: one component under 8-connectivity
    assert regions_ref.label_ref(checker)[1] == 1
    assert regions_ref.label_ref(np.zeros((5, 7), bool))[1] == 0


# ---- the regions rule: the worked example ------------------------------------------------------------------------------------
def _discs():
    H, W = 720, 1280
    yy, xx = np.mgrid[0:H, 0:W]
    S = np.zeros((H, W), bool)
    for cy, cx, r in [(200, 300, 60), (500, 1000, 80), (520, 1100, 30), (100, 900, 3)]:
        S |= (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
    return S


def test_worked_example_components():
    _, n, table = regions_ref.components_of(_discs())
    assert n == 3
    assert table == ((98, 102, 898, 902, 25), (141, 259, 241, 359, 11277), (421, 579, 921, 1129, 22692))


@pytest.mark.parametrize("kw,h,w,origins,members", [
    (dict(context=1.0, padding=0), 160, 216, ((21, 793), (121, 193), (421, 918)), ((1,), (2,), (3,))),
    (dict(context=1.5, padding=32), 304, 384, ((0, 709), (49, 109), (349, 834)), ((1,), (2,), (3,))),
    (dict(context=1.5, padding=32, min_area=50), 304, 384, ((49, 109), (349, 834)), ((2,), (3,))),
    (dict(context=1.5, padding=32, max_regions=2), 312, 1064, ((23, 40), (345, 216)), ((1, 2), (3,))),
    (dict(context=1.0, padding=0, max_regions=1), 488, 896, ((95, 238),), ((1, 2, 3),)),
])
def test_worked_example_rows(kw, h, w, origins, members):
    comps = regions_ref.components_of(_discs())
    r = detail.plan_regions(comps, 720, 1280, multiple_of=8, target=0, **kw)
    assert (r.H, r.W, r.h, r.w, r.oh, r.ow) == (720, 1280, h, w, h, w)
    assert r.origins == origins and r.members == members and len(r) == len(origins)
    assert r.region(0) == detail.Region(origins[0][0], origins[0][1], h, w, h, w, 720, 1280)
    assert r == regions_ref.plan_regions_ref(comps[1], comps[2], 720, 1280, kw["context"], kw["padding"], 8, 0,
                                             kw.get("min_area", 1), kw.get("max_regions", 8))
    if kw.get("max_regions") == 1:                                      # the last row: plan_region of the mask's bounding box
        assert r.region(0) == detail.plan_region((98, 579, 241, 1129), 720, 1280, 1.0, 0, 8, 0)
    with pytest.raises(dataclasses.FrozenInstanceError):
        r.h = 1


def test_working_size_is_one_scale_for_all_regions():
    comps = regions_ref.components_of(_discs())
    r = detail.plan_regions(comps, 720, 1280, 1.5, 32, 8, 1024)
    # h x w = 304 x 384, L = 384: oh = floor((2*304*1024 + 3072) / 6144) = 101 -> 808 (810.67 / 8 = 101.3), ow = 1024
    assert (r.h, r.w, r.oh, r.ow) == (304, 384, 808, 1024) and r.resampled
    assert all(r.region(i).oh == 808 for i in range(len(r)))


# ---- the regions rule: properties over random masks -----------------------------------------------------------------------------
def _bbox_of(table):
    t = np.array(table)
    return (int(t[:, 0].min()), int(t[:, 1].max()), int(t[:, 2].min()), int(t[:, 3].max()))


def test_rule_properties_over_random_masks():
    rng = np.random.default_rng(2024)
    done = compared = 0
    while done < 240:
        H, W = int(rng.integers(8, 301)), int(rng.integers(8, 301))
        density = (0.001, 0.01, 0.05)[done % 3]
        context = (1.0, 1.5, 3.0)[(done // 3) % 3]
        padding, max_regions = int(rng.integers(0, 20)), int(rng.integers(1, 6))
        m, target, min_area = (8, 8, 16, 1)[done % 4], (0, 0, 256)[done % 3], (1, 1, 2)[done % 3]
        S = _random_set(rng, H, W, density)
        _, n, table = regions_ref.components_of(S)
        if n == 0 or not any(row[4] >= min_area for row in table):
            with pytest.raises(ValueError, match="empty" if n == 0 else "min_area"):
                detail.plan_regions((n, table), H, W, context, padding, m, target, min_area, max_regions)
            if n:
                done += 1
            continue
        args = (H, W, context, padding, m, target, min_area, max_regions)
        r = detail.plan_regions((n, table), *args)
        assert r == detail.plan_regions((n, table), *args)                       # deterministic
        assert 1 <= len(r) <= max_regions and len(r.members) == len(r.origins)
        for y0, x0 in r.origins:                                                 # every window lies inside the image
            assert 0 <= y0 and y0 + r.h <= H and 0 <= x0 and x0 + r.w <= W
        kept = sorted(label for label, row in enumerate(table, 1) if row[4] >= min_area)
        assert sorted(label for mem in r.members for label in mem) == kept       # a partition of exactly the kept labels
        assert all(list(mem) == sorted(mem) for mem in r.members)
        assert [mem[0] for mem in r.members] == sorted(mem[0] for mem in r.members)
        for i, mem in enumerate(r.members):                                      # a region's window holds its members' boxes
            for label in mem:
                r0, r1, c0, c1, _ = table[label - 1]
                y0, x0 = r.origins[i]
                assert y0 <= r0 and r1 < y0 + r.h and x0 <= c0 and c1 < x0 + r.w
        one = detail.plan_regions((n, table), H, W, context, padding, m, target, 1, 1)
        assert len(one) == 1 and one.members == (tuple(range(1, n + 1)),)
        assert one.region(0) == detail.plan_region(_bbox_of(table), H, W, context, padding, m, target)
        if n <= 60:                                                              # the rule's text, pair by pair
            assert r == regions_ref.plan_regions_ref(n, table, *args)
            compared += 1
        done += 1
    assert compared >= 60


def test_overflow_falls_back_to_the_bounding_box():
    cap = _cabi.LP_DETAIL_MAX_COMPONENTS
    table = tuple((0, 0, i % 100, i % 100, 1) for i in range(cap))              # a truncated table
    r = detail.plan_regions((cap + 5, table), 64, 100, 1.5, 4, 8, 0, 64, 3, bbox=(2, 40, 10, 90))
    want = detail.plan_region((2, 40, 10, 90), 64, 100, 1.5, 4, 8, 0)
    assert len(r) == 1 and r.region(0) == want and r.members == (tuple(range(1, cap + 6)),)
    with pytest.raises(ValueError, match="bbox"):
        detail.plan_regions((cap + 5, table), 64, 100)


def test_plan_regions_rejects_bad_arguments():
    table = ((1, 2, 3, 4, 4),)
    with pytest.raises(ValueError, match="empty"):
        detail.plan_regions((0, ()), 64, 48)
    with pytest.raises(ValueError, match="min_area"):
        detail.plan_regions((1, table), 64, 48, min_area=5)
    for kw in ({"context": 0.9}, {"padding": -1}, {"multiple_of": 0}, {"target": -8}, {"min_area": 0}, {"max_regions": 0}):
        with pytest.raises(ValueError):
            detail.plan_regions((1, table), 64, 48, **kw)
    with pytest.raises(ValueError):
        detail.plan_regions((1, ((1, 64, 3, 4, 4),)), 64, 48)
    with pytest.raises(ValueError):
        detail.plan_regions((2, table), 64, 48)


# ---- Python API: no CPU fallback ------------------------------------------------------------------------------------------------
def test_region_functions_refuse_cpu_tensors():
    img, mask = torch.zeros(1, 16, 16, 3), torch.zeros(1, 16, 16)
    regions = detail.plan_regions((1, ((2, 5, 2, 5, 16),)), 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        detail.mask_components(mask)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        detail.crop_regions(img, mask, regions)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        detail.stitch_regions(img, img[:, :8, :8], mask, regions, None, 3)
    with pytest.raises(ValueError):
        detail.stitch_regions(img, img, mask, regions, None, 4)
    with pytest.raises(ValueError):
        detail.crop_regions(img, mask, regions, None, "nearest")


# ---- nodes ----------------------------------------------------------------------------------------------------------------------
def test_region_nodes_protocol_and_own_mappings():
    from lanpaint_amd import detail_nodes, detail_region_nodes
    crop, stitch = detail_region_nodes.LanPaint_DetailerCropRegions, detail_region_nodes.LanPaint_DetailerStitchRegions
    assert detail_region_nodes.NODE_CLASS_MAPPINGS == {"LanPaint_DetailerCropRegions": crop,
                                                       "LanPaint_DetailerStitchRegions": stitch}
    assert set(detail_region_nodes.NODE_DISPLAY_NAME_MAPPINGS) == set(detail_region_nodes.NODE_CLASS_MAPPINGS)
    assert len(detail_nodes.NODE_CLASS_MAPPINGS) == 2                            # the existing module is left alone
    req = crop.INPUT_TYPES()["required"]
    old = detail_nodes.LanPaint_DetailerCrop.INPUT_TYPES()["required"]
    assert list(req) == list(old) + ["min_area", "max_regions"]
    assert all(req[name] == old[name] for name in old if name != "mask") and req["mask"][0] == "MASK"
    assert req["min_area"][0] == "INT" and req["min_area"][1]["default"] == 64 and req["min_area"][1]["min"] == 1
    assert req["max_regions"][0] == "INT" and req["max_regions"][1] == {**req["max_regions"][1], "default": 8, "min": 1, "max": 64}
    assert crop.RETURN_TYPES == ("IMAGE", "MASK", "LANPAINT_STITCH_REGIONS", "INT") and crop.FUNCTION == "crop"
    assert crop.RETURN_NAMES == ("cropped_image", "cropped_mask", "stitch", "region_count")
    req = stitch.INPUT_TYPES()["required"]
    assert list(req) == ["stitch", "image", "blend_overlap"] and req["stitch"][0] == "LANPAINT_STITCH_REGIONS"
    assert req["blend_overlap"][1] == {**req["blend_overlap"][1], "min": 1, "max": 51, "step": 2}
    assert stitch.RETURN_TYPES == ("IMAGE",) and stitch.FUNCTION == "stitch"
    for cls in (crop, stitch):
        assert callable(getattr(cls, cls.FUNCTION)) and cls.CATEGORY == "image"
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            crop().crop(torch.zeros(1, 16, 16, 3), torch.zeros(1, 16, 16))


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
def test_region_entries_reject_bad_arguments_without_a_device(hip_lib):
    C, E, U, A = ctypes, _cabi.LP_E_INVALID, _cabi.LP_E_UNSUPPORTED, _cabi.LP_E_ALIGN
    p = C.c_void_p(256)                                    # never dereferenced: validation comes before any HIP call
    ws = _cabi.lp_components_ws_bytes(8, 8)
    assert ws == 4100 and _cabi.lp_components_ws_bytes(720, 1280) == 900 * 4100
    for args in ((None, 1, 8, 8, p, p, p, ws), (p, 1, 8, 8, None, p, p, ws), (p, 1, 8, 8, p, None, p, ws),
                 (p, 1, 8, 8, p, p, None, ws), (p, 0, 8, 8, p, p, p, ws), (p, 1, 0, 8, p, p, p, ws), (p, 1, 8, -2, p, p, p, ws),
                 (p, 1, _cabi.LP_DETAIL_MAX_SIDE + 1, 8, p, p, p, 1 << 40), (p, 1, 8, 8, p, p, p, ws - 1),
                 (p, 1, 33, 32, p, p, p, ws)):
        assert hip_lib.lp_mask_components(*args, None) == E, args
    assert hip_lib.lp_mask_components(p, 1, 8, 8, p, p, C.c_void_p(264), ws, None) == A
    assert hip_lib.lp_mask_components(p, 65536, 8, 8, p, p, p, ws, None) == U

    assert hip_lib.lp_detail_resample_regions(None, None) == E
    good = dict(batch=2, src_h=32, src_w=40, channels=3, regions=3, win_h=16, win_w=24, owner_len=0, out_h=32, out_w=48,
                ksize_x=3, ksize_y=3, origins=p, src=p, bounds_x=p, weights_x=p, bounds_y=p, weights_y=p, dst=p)
    for change in ({"batch": 0}, {"src_h": 0}, {"channels": 0}, {"channels": 65}, {"win_h": 0}, {"win_w": -1}, {"win_w": 41},
                   {"win_h": 33}, {"regions": 0}, {"regions": _cabi.LP_DETAIL_MAX_REGIONS + 1}, {"origins": None},
                   {"out_h": 0}, {"out_w": _cabi.LP_DETAIL_MAX_SIDE + 1}, {"ksize_x": 0}, {"ksize_y": -1}, {"src": None},
                   {"dst": None}, {"bounds_x": None}, {"weights_y": None},
                   {"labels": p, "owner": p, "owner_len": 4, "scratch": p},                 # labels with three channels
                   {"channels": 1, "labels": p, "owner": None, "owner_len": 4, "scratch": p},
                   {"channels": 1, "labels": p, "owner": p, "owner_len": 0, "scratch": p},
                   {"channels": 1, "labels": p, "owner": p, "owner_len": 4, "scratch": None}):
        d = _cabi.LpDetailResampleRegionsDesc(**{**good, **change})
        assert hip_lib.lp_detail_resample_regions(C.byref(d), None) == E, change
    R = _cabi.LpDetailResampleRegionsDesc
    assert hip_lib.lp_detail_resample_regions(C.byref(R(**{**good, "dst": 260})), None) == A
    assert hip_lib.lp_detail_resample_regions(C.byref(R(**{**good, "channels": 1, "labels": p, "owner": p, "owner_len": 4,
                                                           "scratch": 260})), None) == A
    assert hip_lib.lp_detail_resample_regions(C.byref(R(**{**good, "batch": 21846})), None) == U      # 3 * 21846 > 65535

    assert hip_lib.lp_detail_stitch_regions(None, None) == E
    origins = (C.c_int32 * 6)(4, 8, 0, 0, 16, 16)          # on the host: this entry reads them
    bad_origins = (C.c_int32 * 6)(4, 8, 0, 0, 17, 16)      # the third window leaves the image
    at = lambda a: C.cast(a, C.c_void_p)                    # noqa: E731
    good = dict(batch=2, height=32, width=40, channels=3, regions=3, win_h=16, win_w=24, k=9, mask_batch=1, owner_len=0,
                origins=at(origins), mask=p, original=p, detail=p, out=C.c_void_p(512))
    for change in ({"batch": 0}, {"height": 0}, {"width": _cabi.LP_DETAIL_MAX_SIDE + 1}, {"channels": 0}, {"win_h": 0},
                   {"win_h": 17}, {"win_w": 25}, {"regions": 0}, {"regions": 65}, {"origins": None},
                   {"origins": at(bad_origins)}, {"k": 0}, {"k": 8}, {"k": 53}, {"mask_batch": 3}, {"mask": None},
                   {"original": None}, {"detail": None}, {"out": None}, {"out": p}, {"labels": p, "owner": None},
                   {"labels": p, "owner": p, "owner_len": 0}):
        d = _cabi.LpDetailStitchRegionsDesc(**{**good, **change})
        assert hip_lib.lp_detail_stitch_regions(C.byref(d), None) == E, change
    d = _cabi.LpDetailStitchRegionsDesc(**{**good, "batch": 65536})
    assert hip_lib.lp_detail_stitch_regions(C.byref(d), None) == U
