"""The per-subject Detailer, the parts that need no device: the subjects rule's worked answers, its plain restatement
(tests/subjects_ref.py) and its properties over generated box lists, the identity with plan_track, the argument checks of the
four C entries (made before any HIP call), and the nodes' protocol.  Layouts, constants and names against the header are
tests/test_cabi_mirror.py's, for the whole C ABI."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch
from hypothesis import given, settings, strategies as st

from lanpaint_amd import _cabi, detail, detail_subjects
from tests import subjects_ref

CAP = _cabi.LP_DETAIL_MAX_COMPONENTS


def _absent(H, W):
    return (H, -1, W, -1)                                   # what lp_subject_boxes writes for a frame the subject is not in


# ---- known answers, computed by hand from the rule in detail_subjects.py's docstring ---------------------------------------------------
def _two_subjects():
    """100 x 400, 5 frames.  Subject 0: a 20 x 20 box at rows 40..59 whose columns start at 10 and move right 10 a frame.
    Subject 1: a 12 x 12 box at rows 10..21 whose columns start at 300 and move left 10 a frame, absent from frame 2."""
    a = [(40, 59, 10 + 10 * f, 29 + 10 * f) for f in range(5)]
    b = [(10, 21, 300 - 10 * f, 311 - 10 * f) for f in range(5)]
    b[2] = _absent(100, 400)
    return [a, b]


def test_two_subjects_share_the_largest_side_and_each_follows_its_own_path():
    # size: the largest side over both subjects is 20 on both axes; g = 0, n = 20 -> need = 24: h = w = 24 for both.
    # subject 0, rows: s = 100, lo = (100 - 24) // 2 = 38, contain [36, 40] holds.  cols: s_f = 40 + 20 f, lo = 8 + 10 f.
    # subject 1, rows: s = 32, lo = (32 - 24) // 2 = 4, contain [-2, 10] holds.  cols: s_f = 612 - 20 f, lo = 294 - 10 f;
    #   frame 2 is bridged: s = 592 + ((552 - 592) * 1) // 2 = 572, lo = 274 -- on the line, as a constant speed must give.
    sub = detail_subjects.plan_subjects(((1,), (2,)), _two_subjects(), 100, 400, 1.0, 0, 8, 0, 1)
    assert (sub.H, sub.W, sub.h, sub.w, sub.oh, sub.ow) == (100, 400, 24, 24, 24, 24) and not sub.resampled
    assert sub.frames == 5 and sub.subjects == 2 and len(sub) == 10 and sub.members == ((1,), (2,))
    assert sub.origins == tuple((38, 8 + 10 * f) for f in range(5)) + tuple((4, 294 - 10 * f) for f in range(5))
    assert sub.window(1, 3) == detail.Region(4, 264, 24, 24, 24, 24, 100, 400) == sub.region(1 * 5 + 3)
    with pytest.raises(dataclasses.FrozenInstanceError):
        sub.h = 1


def test_a_small_subject_gets_the_large_subjects_window_size_and_the_working_size_is_one():
    # context 1.5, padding 4, M = 8, target 64.  side = 20: g = 4 + ceil(500 * 20 / 2000) = 9, n = 38 -> need = 40.
    # (oh, ow): L = 40, floor((2 * 40 * 64 + 40 * 8) / (2 * 40 * 8)) * 8 = floor(8.5) * 8 = 64.
    # subject 1, rows: lo = (32 - 40) // 2 = -4 -> clamp 0.  cols frame 0: (612 - 40) // 2 = 286.
    sub = detail_subjects.plan_subjects(((1,), (2,)), _two_subjects(), 100, 400, 1.5, 4, 8, 64, 1)
    assert (sub.h, sub.w, sub.oh, sub.ow) == (40, 40, 64, 64) and sub.resampled
    assert sub.origins[5] == (0, 286) and sub.origins[0] == (30, 0 + (40 - 40) // 2)      # subject 0: (100 - 40) // 2, (40 - 40) // 2


def test_keep_is_by_mean_area_over_a_components_life():
    # A lives 5 frames with volume 2000 (mean 400); B 2 frames with 60 (mean 30); C one frame with 50.
    table = ((0, 4, 10, 29, 10, 69, 2000), (2, 3, 50, 55, 100, 105, 60), (0, 0, 80, 89, 200, 204, 50))
    assert detail_subjects.group_subjects((3, table), 1, 8) == ((1,), (2,), (3,))
    assert detail_subjects.group_subjects((3, table), 30, 8) == ((1,), (2,), (3,))       # 60 >= 30 * 2
    assert detail_subjects.group_subjects((3, table), 31, 8) == ((1,), (3,))             # 60 < 62, 50 >= 31
    assert detail_subjects.group_subjects((None, 3, table), 51, 8) == ((1,),)            # the 3-tuple is taken too
    with pytest.raises(ValueError, match="min_area = 401 leaves none of the mask's 3 components: there is no region to detail"):
        detail_subjects.group_subjects((3, table), 401, 8)
    with pytest.raises(ValueError, match="the mask is empty: there is no region to detail"):
        detail_subjects.group_subjects((0, ()), 1, 8)
    with pytest.raises(ValueError):
        detail_subjects.group_subjects((3, table[:2]), 1, 8)
    for bad in ((0, 4), (4, 0)):
        with pytest.raises(ValueError):
            detail_subjects.group_subjects((3, table), *bad)


def _row(f0, f1, r0, r1, c0, c1):
    return (f0, f1, r0, r1, c0, c1, (f1 - f0 + 1) * (r1 - r0 + 1) * (c1 - c0 + 1))


def test_limit_merges_the_smallest_union_box_and_breaks_ties_to_the_lowest_pair():
    # union products over 5 frames: AB = 5 * 10 * 30 = 1500, AC = 5 * 60 * 10 = 3000, BC = 5 * 60 * 30 = 9000
    a, b, c = _row(0, 4, 0, 9, 0, 9), _row(0, 4, 0, 9, 20, 29), _row(0, 4, 50, 59, 0, 9)
    assert detail_subjects.group_subjects((3, (a, b, c)), 1, 2) == ((1, 2), (3,))
    assert detail_subjects.group_subjects((3, (a, b, c)), 1, 1) == ((1, 2, 3),)
    # AB = AC = 1500: the tie goes to the lowest j
    c = _row(0, 4, 20, 29, 0, 9)
    assert detail_subjects.group_subjects((3, (a, b, c)), 1, 2) == ((1, 2), (3,))
    # AC = BC = 5 * 10 * 60 = 3000 < AB = 5500: the tie goes to the lowest i; subjects stay ordered by smallest member
    b, c = _row(0, 4, 0, 9, 100, 109), _row(0, 4, 0, 9, 50, 59)
    assert detail_subjects.group_subjects((3, (a, b, c)), 1, 2) == ((1, 3), (2,))
    # the frame extent counts: B is nearer in space, C nearer in time.  AB = 10 * 10 * 30 = 3000, AC = 1 * 10 * 100 = 1000
    a, b, c = _row(0, 0, 0, 9, 0, 9), _row(9, 9, 0, 9, 20, 29), _row(0, 0, 0, 9, 90, 99)
    assert detail_subjects.group_subjects((3, (a, b, c)), 1, 2) == ((1, 3), (2,))


def test_there_is_no_close_step():
    """Two subjects whose windows overlap in every frame stay two (the regions rule would merge them)."""
    boxes = [[(10, 19, 10, 19)] * 3, [(10, 19, 24, 33)] * 3]           # 4 columns apart; windows of 16 overlap
    sub = detail_subjects.plan_subjects(((1,), (2,)), boxes, 64, 64, 1.0, 0, 8, 0, 1)
    assert sub.subjects == 2 and (sub.h, sub.w) == (16, 16)
    assert sub.origins[0] == (7, 7) and sub.origins[3] == (7, 21) and sub.origins[0][1] + sub.w > sub.origins[3][1]
    table = (_row(0, 2, 10, 19, 10, 19), _row(0, 2, 10, 19, 24, 33))
    assert detail_subjects.group_subjects((2, table), 1, 4) == ((1,), (2,))


def test_past_the_cap_one_subject_owns_every_label_and_the_plan_is_plan_tracks():
    n = CAP + 904
    members = detail_subjects.group_subjects((n, ()), 64, 4)                  # min_area and the table play no part
    assert members == (tuple(range(1, n + 1)),)
    boxes = [(3, 90, 5 + f, 380 - f) for f in range(6)]
    sub = detail_subjects.plan_subjects(members, [boxes], 100, 400, 1.25, 4, 8, 128, 3)
    t = detail.plan_track(boxes, 100, 400, 1.25, 4, 8, 128, 3)
    assert (sub.H, sub.W, sub.h, sub.w, sub.oh, sub.ow, sub.origins) == (t.H, t.W, t.h, t.w, t.oh, t.ow, t.origins)


# ---- generated box lists ------------------------------------------------------------------------------------------------------------
@st.composite
def _jobs(draw, max_subjects=4):
    H, W = draw(st.integers(8, 200)), draw(st.integers(8, 200))
    S, F = draw(st.integers(1, max_subjects)), draw(st.integers(1, 9))
    boxes = []
    for _ in range(S):
        sub = []
        for f in range(F):
            if draw(st.integers(0, 3)) == 0:
                sub.append(_absent(H, W))
                continue
            r0, c0 = draw(st.integers(0, H - 1)), draw(st.integers(0, W - 1))
            sub.append((r0, draw(st.integers(r0, min(H - 1, r0 + 40))), c0, draw(st.integers(c0, min(W - 1, c0 + 40)))))
        if all(b[1] < b[0] for b in sub):
            r0, c0 = draw(st.integers(0, H - 1)), draw(st.integers(0, W - 1))
            sub[draw(st.integers(0, F - 1))] = (r0, r0, c0, c0)
        boxes.append(sub)
    args = (draw(st.sampled_from([1.0, 1.1, 1.5, 2.0])), draw(st.integers(0, 20)), draw(st.sampled_from([1, 8, 16])),
            draw(st.sampled_from([0, 64, 100])), draw(st.sampled_from([1, 3, 9])))
    return H, W, boxes, args


@settings(max_examples=150, deadline=None)
@given(_jobs())
def test_plan_subjects_equals_the_restatement_and_contains_every_box(job):
    H, W, boxes, args = job
    members = tuple((s + 1,) for s in range(len(boxes)))
    sub = detail_subjects.plan_subjects(members, boxes, H, W, *args)
    assert (sub.H, sub.W, sub.h, sub.w, sub.oh, sub.ow, sub.origins) == subjects_ref.plan_subjects_ref(boxes, H, W, *args)
    F = sub.frames
    assert len(sub.origins) == len(boxes) * F and 0 < sub.h <= H and 0 < sub.w <= W
    for s, row in enumerate(boxes):
        for f, (r0, r1, c0, c1) in enumerate(row):
            y0, x0 = sub.origins[s * F + f]
            assert 0 <= y0 <= H - sub.h and 0 <= x0 <= W - sub.w
            if r1 >= r0:                                    # containment: whatever `smooth`, a subject's box is inside its window
                assert y0 <= r0 and r1 < y0 + sub.h and x0 <= c0 and c1 < x0 + sub.w, (s, f)


@settings(max_examples=100, deadline=None)
@given(_jobs(max_subjects=1))
def test_one_subject_is_plan_track(job):
    H, W, boxes, args = job
    sub = detail_subjects.plan_subjects(((1,),), boxes, H, W, *args)
    t = detail.plan_track(boxes[0], H, W, *args)
    assert (sub.H, sub.W, sub.h, sub.w, sub.oh, sub.ow, sub.origins) == (t.H, t.W, t.h, t.w, t.oh, t.ow, t.origins)
    assert sub.frames == len(t) and [sub.window(0, f) for f in range(len(t))] == [t.region(f) for f in range(len(t))]


@settings(max_examples=100, deadline=None)
@given(st.lists(st.tuples(st.integers(0, 5), st.integers(0, 3), st.integers(0, 40), st.integers(0, 12), st.integers(0, 40),
                          st.integers(0, 12), st.integers(1, 300)), min_size=1, max_size=9),
       st.integers(1, 40), st.integers(1, 5))
def test_group_subjects_equals_the_restatement(rows, min_area, max_subjects):
    table = tuple((f0, f0 + df, r0, r0 + dr, c0, c0 + dc, vol) for f0, df, r0, dr, c0, dc, vol in rows)
    try:
        want = subjects_ref.group_subjects_ref(len(table), table, min_area, max_subjects, CAP)
    except ValueError:
        with pytest.raises(ValueError):
            detail_subjects.group_subjects((len(table), table), min_area, max_subjects)
        return
    got = detail_subjects.group_subjects((len(table), table), min_area, max_subjects)
    assert got == want and len(got) <= max_subjects
    assert [m[0] for m in got] == sorted(m[0] for m in got) and all(list(m) == sorted(m) for m in got)


def test_the_labelling_restatement_numbers_components_in_raster_order_of_first_voxel():
    rng = np.random.default_rng(5)
    for density in (0.1, 0.3):
        S = rng.random((4, 9, 11)) < density
        labels, n, table = subjects_ref.label_frames_ref(S)
        assert n == table.shape[0] and int(table[:, 6].sum()) == int(S.sum()) and np.array_equal(labels != 0, S)
        for i in range(n):
            f, y, x = np.nonzero(labels == i + 1)
            assert tuple(table[i]) == (f.min(), f.max(), y.min(), y.max(), x.min(), x.max(), f.size)
    S = np.zeros((3, 4, 4), bool)
    S[0, 0, 0] = S[1, 1, 1] = S[2, 3, 3] = True                    # a diagonal step in time joins; (1,1,1) -> (2,3,3) does not
    assert subjects_ref.label_frames_ref(S)[1] == 2


# ---- argument checks of the planners and wrappers ------------------------------------------------------------------------------------
def test_plan_subjects_rejects_bad_arguments():
    boxes = _two_subjects()
    good = dict(members=((1,), (2,)), boxes=boxes, H=100, W=400)
    detail_subjects.plan_subjects(**good)
    for change in ({"members": ((1,),)}, {"members": ()}, {"members": ((1,), ())}, {"members": ((0,), (2,))},
                   {"boxes": [boxes[0], boxes[1][:4]]}, {"boxes": [boxes[0], [_absent(100, 400)] * 5]},
                   {"boxes": [boxes[0], [(10, 100, 0, 5)] * 5]}, {"H": 0}, {"context": 0.9}, {"padding": -1},
                   {"multiple_of": 0}, {"target": -1}, {"smooth": 2}, {"smooth": 0}, {"smooth": True},
                   {"members": tuple((i + 1,) for i in range(65)), "boxes": [boxes[0]] * 65}):
        with pytest.raises(ValueError):
            detail_subjects.plan_subjects(**{**good, **change})


def test_wrappers_refuse_cpu_tensors_and_a_one_plane_mask():
    img, mask = torch.zeros(2, 16, 16, 3), torch.zeros(2, 16, 16)
    labels = torch.zeros(2, 16, 16, dtype=torch.int32)
    sub = detail_subjects.Subjects(16, 16, 8, 8, 8, 8, ((0, 0), (4, 4)), 2, ((1,),))
    if not torch.cuda.is_available():
        for call in (lambda: detail_subjects.mask_components_frames(mask),
                     lambda: detail_subjects.subject_boxes(labels, ((1,),)),
                     lambda: detail_subjects.crop_subjects(img, mask, sub, None),
                     lambda: detail_subjects.stitch_subjects(img, img[:, :8, :8], mask, sub, None, 3)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call()
    with pytest.raises(ValueError, match="region nodes"):
        detail_subjects._frame_mask(mask[:1], 2, 16, 16)
    with pytest.raises(ValueError, match="region nodes"):
        detail_subjects._frame_mask(mask[0], 2, 16, 16)
    with pytest.raises(ValueError):
        detail_subjects._frame_mask(torch.zeros(3, 16, 16), 2, 16, 16)
    for bad in (dataclasses.replace(sub, origins=sub.origins[:1]), dataclasses.replace(sub, origins=((0, 0), (9, 0))),
                dataclasses.replace(sub, origins=((0, -1), (0, 0))), dataclasses.replace(sub, H=32),
                dataclasses.replace(sub, frames=1), dataclasses.replace(sub, h=17)):
        with pytest.raises(ValueError):
            detail_subjects._check_subjects(bad, None, 2, 16, 16)
    detail_subjects._check_subjects(sub, None, 2, 16, 16)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_subject_entries_reject_bad_arguments_without_a_device(hip_lib):
    C, E, U, A = ctypes, _cabi.LP_E_INVALID, _cabi.LP_E_UNSUPPORTED, _cabi.LP_E_ALIGN
    p = C.c_void_p(256)                                    # never dereferenced: validation comes before any HIP call
    side = _cabi.LP_DETAIL_MAX_SIDE
    ws = _cabi.lp_components_frames_ws_bytes
    for args in ((None, 2, 8, 8, p, p, p, ws(2, 8, 8)), (p, 2, 8, 8, None, p, p, ws(2, 8, 8)), (p, 2, 8, 8, p, None, p, ws(2, 8, 8)),
                 (p, 2, 8, 8, p, p, None, ws(2, 8, 8)), (p, 0, 8, 8, p, p, p, ws(2, 8, 8)), (p, -1, 8, 8, p, p, p, ws(2, 8, 8)),
                 (p, 2, 0, 8, p, p, p, ws(2, 8, 8)), (p, 2, 8, side + 1, p, p, p, 1 << 40), (p, 2, 8, 8, p, p, p, ws(2, 8, 8) - 1),
                 (p, 3, 8, 8, p, p, p, 0)):
        assert hip_lib.lp_mask_components_frames(*args, None) == E, args
    assert hip_lib.lp_mask_components_frames(p, 2, 8, 8, p, p, C.c_void_p(260), ws(2, 8, 8), None) == A
    assert hip_lib.lp_mask_components_frames(p, 65536, 8, 8, p, p, p, ws(65536, 8, 8), None) == U
    assert hip_lib.lp_mask_components_frames(p, 2, side, side, p, p, p, ws(2, side, side), None) == U       # 2^31 voxels
    assert hip_lib.lp_mask_components_frames(p, 5, 16384, 16384, p, p, p, ws(5, 16384, 16384), None) == U   # just past 2^30
    assert hip_lib.lp_mask_components(p, 1, 0, 8, p, p, p, 1 << 20, None) == E                              # the sibling's codes

    for args in ((None, 2, 8, 8, p, 3, 2, p), (p, 2, 8, 8, None, 3, 2, p), (p, 2, 8, 8, p, 3, 2, None), (p, 0, 8, 8, p, 3, 2, p),
                 (p, 2, 0, 8, p, 3, 2, p), (p, 2, 8, side + 1, p, 3, 2, p), (p, 2, 8, 8, p, 0, 2, p), (p, 2, 8, 8, p, 3, 0, p),
                 (p, 2, 8, 8, p, 3, _cabi.LP_DETAIL_MAX_REGIONS + 1, p)):
        assert hip_lib.lp_subject_boxes(*args, None) == E, args
    assert hip_lib.lp_subject_boxes(p, 65536, 8, 8, p, 3, 2, p, None) == U

    R = _cabi.LpDetailResampleSubjectsDesc
    assert hip_lib.lp_detail_resample_subjects(None, None) == E
    good = dict(batch=2, src_h=32, src_w=40, channels=3, subjects=2, win_h=16, win_w=24, owner_len=0, out_h=32, out_w=48,
                ksize_x=3, ksize_y=3, origins=p, src=p, bounds_x=p, weights_x=p, bounds_y=p, weights_y=p, dst=p)
    for change in ({"batch": 0}, {"src_h": 0}, {"src_w": side + 1}, {"channels": 0}, {"channels": 65}, {"subjects": 0},
                   {"subjects": _cabi.LP_DETAIL_MAX_REGIONS + 1}, {"win_h": 0}, {"win_w": -1}, {"win_w": 41}, {"win_h": 33},
                   {"origins": None}, {"out_h": 0}, {"out_w": side + 1}, {"ksize_x": 0}, {"ksize_y": -1}, {"src": None},
                   {"dst": None}, {"bounds_x": None}, {"weights_y": None},
                   {"labels": p, "owner": p, "owner_len": 2, "scratch": p},                       # labels need channels == 1
                   {"channels": 1, "labels": p, "owner": None, "owner_len": 2, "scratch": p},
                   {"channels": 1, "labels": p, "owner": p, "owner_len": 0, "scratch": p},
                   {"channels": 1, "labels": p, "owner": p, "owner_len": 2, "scratch": None}):
        assert hip_lib.lp_detail_resample_subjects(C.byref(R(**{**good, **change})), None) == E, change
    assert hip_lib.lp_detail_resample_subjects(C.byref(R(**{**good, "dst": 260})), None) == A
    erased = {**good, "channels": 1, "labels": p, "owner": p, "owner_len": 2, "scratch": 260}
    assert hip_lib.lp_detail_resample_subjects(C.byref(R(**erased)), None) == A
    assert hip_lib.lp_detail_resample_subjects(C.byref(R(**{**good, "batch": 32768})), None) == U      # 2 * 32768 windows

    S = _cabi.LpDetailStitchSubjectsDesc
    assert hip_lib.lp_detail_stitch_subjects(None, None) == E
    good = dict(batch=2, height=32, width=40, channels=3, subjects=2, win_h=16, win_w=24, k=9, owner_len=0, origins=p, mask=p,
                original=p, detail=p, out=C.c_void_p(512))
    for change in ({"batch": 0}, {"height": 0}, {"width": side + 1}, {"channels": 0}, {"channels": 65}, {"subjects": 0},
                   {"subjects": _cabi.LP_DETAIL_MAX_REGIONS + 1}, {"win_h": 0}, {"win_h": 33}, {"win_w": 41}, {"origins": None},
                   {"k": 0}, {"k": 8}, {"k": 53}, {"mask": None}, {"original": None}, {"detail": None}, {"out": None}, {"out": p},
                   {"labels": p, "owner": None, "owner_len": 2}, {"labels": p, "owner": p, "owner_len": 0}):
        assert hip_lib.lp_detail_stitch_subjects(C.byref(S(**{**good, **change})), None) == E, change
    assert hip_lib.lp_detail_stitch_subjects(C.byref(S(**{**good, "batch": 65536})), None) == U


# ---- nodes ----------------------------------------------------------------------------------------------------------------------------
def test_subject_nodes_protocol_and_own_mappings():
    from lanpaint_amd import detail_nodes, detail_region_nodes, detail_subject_nodes, detail_track_nodes
    crop, stitch = detail_subject_nodes.LanPaint_DetailerCropSubjects, detail_subject_nodes.LanPaint_DetailerStitchSubjects
    assert detail_subject_nodes.NODE_CLASS_MAPPINGS == {"LanPaint_DetailerCropSubjects": crop,
                                                        "LanPaint_DetailerStitchSubjects": stitch}
    assert set(detail_subject_nodes.NODE_DISPLAY_NAME_MAPPINGS) == set(detail_subject_nodes.NODE_CLASS_MAPPINGS)
    assert len(detail_track_nodes.NODE_CLASS_MAPPINGS) == 2 and len(detail_region_nodes.NODE_CLASS_MAPPINGS) == 2
    req = crop.INPUT_TYPES()["required"]
    old = detail_track_nodes.LanPaint_DetailerCropTrack.INPUT_TYPES()["required"]
    assert list(req) == ["image", "mask", "context", "padding", "target", "multiple_of", "filter", "smooth", "min_area",
                         "max_subjects"]
    assert list(req) == list(old) + ["min_area", "max_subjects"]
    assert all(req[name] == old[name] for name in old if name != "mask") and req["mask"][0] == "MASK"
    assert req["min_area"][0] == "INT" and req["min_area"][1] == {**req["min_area"][1], "default": 64, "min": 1}
    assert req["max_subjects"][0] == "INT"
    assert req["max_subjects"][1] == {**req["max_subjects"][1], "default": 4, "min": 1, "max": _cabi.LP_DETAIL_MAX_REGIONS}
    assert crop.RETURN_TYPES == ("IMAGE", "MASK", "LANPAINT_STITCH_SUBJECTS", "INT") and crop.FUNCTION == "crop"
    assert crop.RETURN_NAMES == ("cropped_image", "cropped_mask", "stitch", "subject_count")
    assert "clip_frames" in crop.DESCRIPTION and "clip length" in crop.DESCRIPTION
    req = stitch.INPUT_TYPES()["required"]
    assert list(req) == ["stitch", "image", "blend_overlap"] and req["stitch"][0] == "LANPAINT_STITCH_SUBJECTS"
    assert req["blend_overlap"][1] == {**req["blend_overlap"][1], "default": 9, "min": 1, "max": 51, "step": 2}
    assert stitch.RETURN_TYPES == ("IMAGE",) and stitch.RETURN_NAMES == ("image",) and stitch.FUNCTION == "stitch"
    sockets = {detail_nodes.LanPaint_DetailerCrop.RETURN_TYPES[2], detail_region_nodes.LanPaint_DetailerCropRegions.RETURN_TYPES[2],
               detail_track_nodes.LanPaint_DetailerCropTrack.RETURN_TYPES[2]}
    assert "LANPAINT_STITCH_SUBJECTS" not in sockets                               # cannot be wired into the other stitch nodes
    for cls in (crop, stitch):
        assert callable(getattr(cls, cls.FUNCTION)) and cls.CATEGORY == "image"
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            crop().crop(torch.zeros(2, 16, 16, 3), torch.zeros(2, 16, 16))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            stitch().stitch({"original": torch.zeros(2, 16, 16, 3)}, torch.zeros(2, 8, 8, 3), 9)
