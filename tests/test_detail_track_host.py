"""The Detailer that follows a moving mask, the parts that need no device: the track rule's worked answers, its plain
restatement (tests/track_ref.py) and its properties over generated box lists, the argument checks of plan_track and of the three
C entries (made before any HIP call), and the nodes' protocol.  Layouts, constants and names against the header are
tests/test_cabi_mirror.py's, for the whole C ABI."""
import ctypes
import dataclasses

import pytest
import torch
from hypothesis import given, settings, strategies as st

from lanpaint_amd import _cabi, detail
from tests import track_ref


def _empty(H, W):
    return (H, -1, W, -1)                                   # what lp_mask_bbox_frames writes for a plane with nothing set


# ---- known answers, computed by hand from the rule in detail.py's docstring ---------------------------------------------------------
def _moving(frames=9):
    """A 20 x 20 box at rows 40..59 whose columns start at 10 and move 10 pixels a frame, in a 100 x 400 image."""
    return [(40, 59, 10 + 10 * f, 29 + 10 * f) for f in range(frames)]


def test_constant_speed_without_smoothing_keeps_the_box_centred():
    # rows: s = 100, side = 20, g = 0, n = 20 -> need = 24;  lo = (100 - 24) // 2 = 38
    # cols: s_f = 40 + 20 f, n = 24;  lo_f = (40 + 20 f - 24) // 2 = 8 + 10 f; contain [6 + 10 f, 10 + 10 f] holds; 88 <= 400 - 24
    t = detail.plan_track(_moving(), 100, 400, 1.0, 0, 8, 0, 1)
    assert (t.H, t.W, t.h, t.w, t.oh, t.ow) == (100, 400, 24, 24, 24, 24) and not t.resampled and len(t) == 9
    assert t.origins == tuple((38, 8 + 10 * f) for f in range(9))
    assert t.region(3) == detail.Region(38, 38, 24, 24, 24, 24, 100, 400)
    with pytest.raises(dataclasses.FrozenInstanceError):
        t.h = 1


def test_constant_speed_smoothed_over_nine_frames_lags_at_the_ends_and_is_held_by_contain():
    # k = 9, r = 4, k n = 216, s_i = 40 + 20 i, indices clamped to 0..8; lo = (S - 216) // 18, then contain to [6 + 10 f, 10 + 10 f]
    #   f  index sum  S     (S-216)//18  contained
    #   0  10         560   19           10   (<= a0)
    #   1  15         660   24           20
    #   2  21         780   31           30
    #   3  28         920   39           39
    #   4  36         1080  48           48   (the unsmoothed centre: the average over a symmetric span of a linear path)
    #   5  44         1240  56           56
    #   6  51         1380  64           66   (>= a1 + 1 - n)
    #   7  57         1500  71           76
    #   8  62         1600  76           86
    t = detail.plan_track(_moving(), 100, 400, 1.0, 0, 8, 0, 9)
    assert (t.h, t.w) == (24, 24)
    assert t.origins == tuple((38, x) for x in (10, 20, 30, 39, 48, 56, 66, 76, 86))
    one = detail.plan_track(_moving(), 100, 400, 1.0, 0, 8, 0, 1)
    assert t.origins != one.origins and t.origins[4] == one.origins[4]


def test_empty_frames_in_the_middle_and_at_both_ends_are_bridged():
    H, W, e = 32, 64, _empty(32, 64)
    # cols: s_1 = 30, s_4 = 90;  fill 0 -> 30, 2 -> 30 + 60 * 1 // 3 = 50, 3 -> 30 + 60 * 2 // 3 = 70, 5, 6 -> 90
    #       side = 10, g = 2, n = 14 -> need = 16;  lo = (s - 16) // 2 = 7, 7, 17, 27, 37, 37, 37
    # rows: s = 24 everywhere, side = 8, g = 2, n = 12 = need;  lo = 6
    boxes = [e, (8, 15, 10, 19), e, e, (8, 15, 40, 49), e, e]
    t = detail.plan_track(boxes, H, W, 1.0, 2, 4, 0, 1)
    assert (t.h, t.w) == (12, 16)
    assert t.origins == ((6, 7), (6, 7), (6, 17), (6, 27), (6, 37), (6, 37), (6, 37))
    # moving left, so that the floor of a negative quotient shows: s_1 = 90, s_4 = 11 + 19 + 1 = 31
    #       fill 2 -> 90 + (-59 // 3 = -20) = 70, 3 -> 90 + (-118 // 3 = -40) = 50;  lo = 37, 37, 27, 17, (31 - 16) // 2 = 7, 7, 7
    boxes = [e, (8, 15, 40, 49), e, e, (8, 15, 11, 19), e, e]
    t = detail.plan_track(boxes, H, W, 1.0, 2, 4, 0, 1)
    assert t.origins == ((6, 37), (6, 37), (6, 27), (6, 17), (6, 7), (6, 7), (6, 7))
    # working size, one scale: L = 16, oh = (2 * 12 * 64 + 64) // 128 = 12 -> 48, ow = (2 * 16 * 64 + 64) // 128 = 16 -> 64
    t = detail.plan_track(boxes, H, W, 1.0, 2, 4, 64, 1)
    assert (t.h, t.w, t.oh, t.ow) == (12, 16, 48, 64) and t.resampled and t.region(6) == detail.Region(6, 7, 12, 16, 48, 64, H, W)


def test_box_touching_the_image_border_is_clamped_inside():
    # rows [0, 9]: s = 10, side = 10, g = ceil(1000 * 10 / 2000) = 5, n = 20 -> 24; lo = (10 - 24) // 2 = -7 -> clamp 0
    # cols [60, 63]: s = 124, side = 4, g = 2, n = 8; lo = (124 - 8) // 2 = 58 -> clamp 64 - 8 = 56
    t = detail.plan_track([(0, 9, 60, 63)], 64, 64, 2.0, 0, 8, 0, 1)
    assert (t.h, t.w, t.origins) == (24, 8, ((0, 56),))


def test_a_window_that_cannot_reach_a_multiple_stays_as_grown():
    # rows [2, 18] in 20 rows, M = 16: n = 17, need = 32 > 20 -> n = 17; s = 21, lo = (21 - 17) // 2 = 2
    # cols [10, 19]: n = 10 -> 16; s = 30, lo = 7
    t = detail.plan_track([(2, 18, 10, 19)], 20, 100, 1.0, 0, 16, 0, 1)
    assert (t.h, t.w, t.origins) == (17, 16, ((2, 7),))
    # padding 10: rows n = min(37, 20) = 20, need = 32 > 20 -> 20; lo = (21 - 20) // 2 = 0.  cols n = 30 -> 32; lo = -1 -> 0
    t = detail.plan_track([(2, 18, 10, 19)], 20, 100, 1.0, 10, 16, 0, 1)
    assert (t.h, t.w, t.origins) == (20, 32, ((0, 0),))


@pytest.mark.parametrize("smooth", [1, 9])
def test_static_one_plane_mask_gives_one_origin_per_frame(smooth):
    t = detail.plan_track([(8, 15, 10, 19)], 32, 64, 1.0, 2, 4, 0, smooth, frames=5)
    assert len(t) == 5 and (t.h, t.w) == (12, 16) and t.origins == ((6, 7),) * 5
    assert t == detail.plan_track([(8, 15, 10, 19)] * 5, 32, 64, 1.0, 2, 4, 0, smooth)


# ---- the restatement and the properties, over generated box lists --------------------------------------------------------------------
@st.composite
def _cases(draw):
    H, W = draw(st.integers(1, 4096)), draw(st.integers(1, 4096))
    frames = draw(st.integers(1, 14))

    def box():
        r0, c0 = draw(st.integers(0, H - 1)), draw(st.integers(0, W - 1))
        big = draw(st.booleans())
        r1 = draw(st.integers(r0, H - 1 if big else min(H - 1, r0 + 40)))
        c1 = draw(st.integers(c0, W - 1 if big else min(W - 1, c0 + 40)))
        return (r0, r1, c0, c1)

    boxes = [box() if draw(st.integers(0, 3)) else _empty(H, W) for _ in range(frames)]
    if all(b[1] < b[0] for b in boxes):
        boxes[draw(st.integers(0, frames - 1))] = box()
    context = draw(st.sampled_from([1.0, 1.001, 1.25, 1.5, 2.0, 3.333, 8.0]))
    padding = draw(st.integers(0, 64))
    m = draw(st.sampled_from([1, 2, 8, 16, 64, 100]))
    target = draw(st.sampled_from([0, 0, 64, 512, 1024]))
    smooth = 2 * draw(st.integers(0, 10)) + 1
    return boxes, H, W, context, padding, m, target, smooth


@settings(max_examples=400, deadline=None, derandomize=True, database=None)
@given(_cases())
def test_plan_track_equals_the_plain_restatement_and_keeps_its_promises(case):
    boxes, H, W, context, padding, m, target, smooth = case
    t = detail.plan_track(boxes, H, W, context, padding, m, target, smooth)
    assert (t.H, t.W, t.h, t.w, t.oh, t.ow, t.origins) == track_ref.plan_track_ref(boxes, H, W, context, padding, m, target, smooth)
    assert len(t) == len(boxes) and 0 < t.h <= H and 0 < t.w <= W
    assert {(t.region(f).h, t.region(f).w) for f in range(len(t))} == {(t.h, t.w)}    # all windows have one size
    for (r0, r1, c0, c1), (y0, x0) in zip(boxes, t.origins):
        assert 0 <= y0 and y0 + t.h <= H and 0 <= x0 and x0 + t.w <= W            # every window inside the image
        if r1 >= r0:                                                              # a frame's own box inside its window
            assert y0 <= r0 and r1 < y0 + t.h and x0 <= c0 and c1 < x0 + t.w
    # the size is a multiple of M whenever the grown side's next multiple fits the image
    full = [b for b in boxes if b[1] >= b[0]]
    c = int(round(context * 1000))
    for n, N, side in ((t.h, H, max(b[1] - b[0] + 1 for b in full)), (t.w, W, max(b[3] - b[2] + 1 for b in full))):
        grown = min(side + 2 * (padding - (-(c - 1000) * side // 2000)), N)
        need = -(-grown // m) * m
        assert (n == need and n % m == 0) if need <= N else n == grown
    assert (t.oh, t.ow) == (t.h, t.w) if target == 0 else (t.oh % m == 0 and t.ow % m == 0 and min(t.oh, t.ow) >= m)


@settings(max_examples=200, deadline=None, derandomize=True, database=None)
@given(_cases(), st.integers(1, 12))
def test_constant_boxes_give_constant_centred_origins(case, frames):
    boxes, H, W, context, padding, m, target, smooth = case
    box = next(b for b in boxes if b[1] >= b[0])
    t = detail.plan_track([box] * frames, H, W, context, padding, m, target, smooth)
    assert len(set(t.origins)) == 1                                               # for any smooth
    assert t == detail.plan_track([box], H, W, context, padding, m, target, smooth, frames=frames)
    one = detail.plan_track([box] * frames, H, W, context, padding, m, target, 1)
    assert one.origins == t.origins
    # smooth = 1: the window's twice-centre 2 lo + n is the box's s or s - 1, unless the image border pushed the window in
    for lo, n, N, a0, a1 in ((one.origins[0][0], one.h, H, box[0], box[1]), (one.origins[0][1], one.w, W, box[2], box[3])):
        s = a0 + a1 + 1
        assert 2 * lo + n in (s, s - 1) or (lo == 0 and 2 * lo + n > s) or (lo == N - n and 2 * lo + n < s - 1)


# ---- errors ---------------------------------------------------------------------------------------------------------------------------
def test_plan_track_rejects_bad_arguments():
    box = (1, 2, 3, 4)
    with pytest.raises(ValueError, match="the mask is empty"):
        detail.plan_track([_empty(64, 48)] * 3, 64, 48)
    with pytest.raises(ValueError, match="the mask is empty"):
        detail.plan_track([_empty(64, 48)], 64, 48, frames=4)
    for kw in ({"context": 0.9}, {"padding": -1}, {"multiple_of": 0}, {"target": -8}, {"smooth": 0}, {"smooth": 4}, {"smooth": -3},
               {"smooth": 2.5}, {"frames": 3}, {"frames": 0}):
        with pytest.raises(ValueError):
            detail.plan_track([box, box], 64, 48, **kw)
    for bad in ((1, 64, 3, 4), (1, 2, 3, 48), (-1, 2, 3, 4), (1, 2, -2, 4)):
        with pytest.raises(ValueError, match="outside"):
            detail.plan_track([box, bad], 64, 48)
    with pytest.raises(ValueError):
        detail.plan_track([], 64, 48)
    with pytest.raises(ValueError):
        detail.plan_track([box], 0, 48)
    assert len(detail.plan_track([box, box], 64, 48, frames=2)) == 2


def test_track_functions_refuse_cpu_tensors_and_bad_tracks():
    img, mask = torch.zeros(2, 16, 16, 3), torch.zeros(2, 16, 16)
    track = detail.plan_track([(2, 5, 2, 5), (3, 6, 4, 7)], 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        detail.mask_bbox_frames(mask)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        detail.crop_track(img, mask, track)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        detail.stitch_track(img, img[:, :8, :8], mask, track, 3)
    with pytest.raises(ValueError):
        detail.stitch_track(img, img, mask, track, 4)
    with pytest.raises(ValueError):
        detail.crop_track(img, mask, track, "nearest")
    for bad in (dataclasses.replace(track, origins=track.origins[:1]),            # not one origin per image
                dataclasses.replace(track, origins=((0, 0), (9, 0))),             # a window that leaves the image
                dataclasses.replace(track, origins=((0, -1), (0, 0))),
                dataclasses.replace(track, H=32)):
        with pytest.raises(ValueError):
            detail._check_track(bad, 2, 16, 16)
    detail._check_track(track, 2, 16, 16)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_track_entries_reject_bad_arguments_without_a_device(hip_lib):
    C, E, U, A = ctypes, _cabi.LP_E_INVALID, _cabi.LP_E_UNSUPPORTED, _cabi.LP_E_ALIGN
    p = C.c_void_p(256)                                    # never dereferenced: validation comes before any HIP call
    for args in ((None, 1, 8, 8, p), (p, 1, 8, 8, None), (p, 0, 8, 8, p), (p, -1, 8, 8, p), (p, 1, 0, 8, p), (p, 1, 8, -2, p),
                 (p, 1, _cabi.LP_DETAIL_MAX_SIDE + 1, 8, p), (p, 1, 8, _cabi.LP_DETAIL_MAX_SIDE + 1, p)):
        assert hip_lib.lp_mask_bbox_frames(*args, None) == E, args
        assert hip_lib.lp_mask_bbox(*args, None) == E, args                      # the sibling's codes
    assert hip_lib.lp_mask_bbox_frames(p, 65536, 8, 8, p, None) == U == hip_lib.lp_mask_bbox(p, 65536, 8, 8, p, None)

    R = _cabi.LpDetailResampleTrackDesc
    assert hip_lib.lp_detail_resample_track(None, None) == E
    good = dict(batch=2, src_h=32, src_w=40, channels=3, win_h=16, win_w=24, out_h=32, out_w=48, ksize_x=3, ksize_y=3,
                origins=p, src=p, bounds_x=p, weights_x=p, bounds_y=p, weights_y=p, dst=p)
    for change in ({"batch": 0}, {"src_h": 0}, {"src_w": _cabi.LP_DETAIL_MAX_SIDE + 1}, {"channels": 0}, {"channels": 65},
                   {"win_h": 0}, {"win_w": -1}, {"win_w": 41}, {"win_h": 33}, {"origins": None}, {"out_h": 0},
                   {"out_w": _cabi.LP_DETAIL_MAX_SIDE + 1}, {"ksize_x": 0}, {"ksize_y": -1}, {"src": None}, {"dst": None},
                   {"bounds_x": None}, {"weights_x": None}, {"bounds_y": None}, {"weights_y": None}):
        assert hip_lib.lp_detail_resample_track(C.byref(R(**{**good, **change})), None) == E, change
    assert hip_lib.lp_detail_resample_track(C.byref(R(**{**good, "dst": 260})), None) == A
    assert hip_lib.lp_detail_resample_track(C.byref(R(**{**good, "batch": 65536})), None) == U
    same = {**good, "out_h": 16, "out_w": 24, "ksize_x": 0, "ksize_y": 0, "bounds_x": None, "weights_x": None, "bounds_y": None,
            "weights_y": None}                             # a window copy reads no table; only the size checks remain
    assert hip_lib.lp_detail_resample_track(C.byref(R(**{**same, "batch": 65536})), None) == U
    assert hip_lib.lp_detail_resample_track(C.byref(R(**{**same, "origins": None})), None) == E

    S = _cabi.LpDetailStitchTrackDesc
    assert hip_lib.lp_detail_stitch_track(None, None) == E
    good = dict(batch=2, height=32, width=40, channels=3, win_h=16, win_w=24, k=9, mask_batch=1, origins=p, mask=p, original=p,
                detail=p, out=C.c_void_p(512))
    for change in ({"batch": 0}, {"height": 0}, {"width": _cabi.LP_DETAIL_MAX_SIDE + 1}, {"channels": 0}, {"channels": 65},
                   {"win_h": 0}, {"win_h": 33}, {"win_w": 41}, {"origins": None}, {"k": 0}, {"k": 8}, {"k": 53}, {"mask_batch": 3},
                   {"mask_batch": 0}, {"mask": None}, {"original": None}, {"detail": None}, {"out": None}, {"out": p}):
        assert hip_lib.lp_detail_stitch_track(C.byref(S(**{**good, **change})), None) == E, change
    assert hip_lib.lp_detail_stitch_track(C.byref(S(**{**good, "batch": 65536, "mask_batch": 65536})), None) == U


# ---- nodes ----------------------------------------------------------------------------------------------------------------------------
def test_track_nodes_protocol_and_own_mappings():
    from lanpaint_amd import detail_nodes, detail_region_nodes, detail_track_nodes
    crop, stitch = detail_track_nodes.LanPaint_DetailerCropTrack, detail_track_nodes.LanPaint_DetailerStitchTrack
    assert detail_track_nodes.NODE_CLASS_MAPPINGS == {"LanPaint_DetailerCropTrack": crop, "LanPaint_DetailerStitchTrack": stitch}
    assert set(detail_track_nodes.NODE_DISPLAY_NAME_MAPPINGS) == set(detail_track_nodes.NODE_CLASS_MAPPINGS)
    assert len(detail_nodes.NODE_CLASS_MAPPINGS) == 2 and len(detail_region_nodes.NODE_CLASS_MAPPINGS) == 2
    req = crop.INPUT_TYPES()["required"]
    old = detail_nodes.LanPaint_DetailerCrop.INPUT_TYPES()["required"]
    assert list(req) == ["image", "mask", "context", "padding", "target", "multiple_of", "filter", "smooth"]
    assert list(req) == list(old) + ["smooth"]
    assert all(req[name] == old[name] for name in old if name != "mask") and req["mask"][0] == "MASK"   # the crop node's defaults
    assert req["smooth"][0] == "INT"
    assert req["smooth"][1] == {**req["smooth"][1], "default": 9, "min": 1, "max": 129, "step": 2}
    assert "number of frames the window's path is averaged over" in req["smooth"][1]["tooltip"].lower()
    assert crop.RETURN_TYPES == ("IMAGE", "MASK", "LANPAINT_STITCH_TRACK") and crop.FUNCTION == "crop"
    assert crop.RETURN_NAMES == ("cropped_image", "cropped_mask", "stitch")
    req = stitch.INPUT_TYPES()["required"]
    assert list(req) == ["stitch", "image", "blend_overlap"] and req["stitch"][0] == "LANPAINT_STITCH_TRACK"
    assert req["blend_overlap"][1] == {**req["blend_overlap"][1], "default": 9, "min": 1, "max": 51, "step": 2}
    assert stitch.RETURN_TYPES == ("IMAGE",) and stitch.RETURN_NAMES == ("image",) and stitch.FUNCTION == "stitch"
    sockets = {detail_nodes.LanPaint_DetailerCrop.RETURN_TYPES[2], detail_region_nodes.LanPaint_DetailerCropRegions.RETURN_TYPES[2]}
    assert "LANPAINT_STITCH_TRACK" not in sockets                                  # cannot be wired into the other stitch nodes
    for cls in (crop, stitch):
        assert callable(getattr(cls, cls.FUNCTION)) and cls.CATEGORY == "image"
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            crop().crop(torch.zeros(2, 16, 16, 3), torch.zeros(2, 16, 16))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            stitch().stitch({"original": torch.zeros(2, 16, 16, 3)}, torch.zeros(2, 8, 8, 3), 9)
