"""The video mask propagate from several keyframes, the parts that need no device: the plan of the chains against hand-written lists,
the properties the rule promises on the restatement (tests/propagate_keys_ref.py) as bits, exact tracking of whole-pixel shifts
between keys, the quality condition on the moving-disc scenes, the C entries' argument checks (made before any HIP call), the
node's protocol and the no-fallback errors.  Layouts, constants and names against the header are tests/test_cabi_mirror.py's, for
the whole C ABI."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi
from tests import propagate_keys_ref as kref
from tests import propagate_ref as ref
from tests.compare import _f32_bits as _bits, _iou
from tests.propagate_scenes import SCENES, disc_scene, texture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = np.float32(1.0).view(np.uint32)


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------
PLANS = [
    (7, [0], [(0, 0, 1, 6)]),
    (7, [6], [(0, 6, -1, 6)]),
    (7, [3], [(0, 3, -1, 3), (0, 3, 1, 3)]),
    (7, [0, 6], [(0, 0, 1, 5), (1, 6, -1, 5)]),
    (7, [2, 4], [(0, 2, -1, 2), (0, 2, 1, 1), (1, 4, -1, 1), (1, 4, 1, 2)]),
    (7, [2, 3], [(0, 2, -1, 2), (1, 3, 1, 3)]),                       # adjacent keys: the gap has no chain
    (7, [0, 3, 6], [(0, 0, 1, 2), (1, 3, -1, 2), (1, 3, 1, 2), (2, 6, -1, 2)]),
    (7, [1, 5], [(0, 1, -1, 1), (0, 1, 1, 3), (1, 5, -1, 3), (1, 5, 1, 1)]),
    (4, [0, 1, 2, 3], []),                                            # every frame a key
    (1, [0], []),
    (36, list(range(0, 36, 2)), [c for a in range(0, 34, 2) for c in ((a // 2, a, 1, 1), (a // 2 + 1, a + 2, -1, 1))] + [(17, 34, 1, 1)]),
]


@pytest.mark.parametrize("frames,keys,want", PLANS, ids=lambda v: str(v) if isinstance(v, int) else None)
def test_chain_plan_equals_the_hand_written_list(frames, keys, want):
    from lanpaint_amd import propagate_keys
    assert propagate_keys.chain_plan(frames, keys) == want
    assert propagate_keys.chain_plan(frames, tuple(keys)) == want
    assert kref.chain_plan(frames, keys) == want
    covered = sorted(k + d * s for _, k, d, n in want for s in range(1, n + 1))
    inner = [t for a, b in zip(keys, keys[1:]) for t in range(a + 1, b)]
    outer = [t for t in range(frames) if t < keys[0] or t > keys[-1]]
    assert covered == sorted(inner + inner + outer)                    # two chains on an in-between frame, one outside the keys


def test_chain_plan_refuses_bad_key_frames():
    from lanpaint_amd import propagate_keys
    for bad in ([], [3, 1], [1, 1], [0, 7], [-1], [7], [1.0], ["1"], [True], [None], 3, None, [0, 2, 2], [[0]]):
        with pytest.raises(ValueError):
            propagate_keys.chain_plan(7, bad)
    for bad in (0, -1, 2.0, None):
        with pytest.raises(ValueError):
            propagate_keys.chain_plan(bad, [0])


# ---- the properties the rule promises, on the restatement --------------------------------------------------------------------------------
def test_the_merge_one_value_at_a_time():
    far = kref.stab.Q_FAR
    # equal distances give the bits back: |s| >= 1 puts 0.5 + sd beyond the ramp
    for q in (1, 2, 3, 4096, 4097, far, -1, -2, -4096, -far):
        for n, j in ((2, 1), (3, 1), (7, 3), (65535, 1), (65535, 65534)):
            got = kref.merge(np.array([[q]]), np.array([[q]]), n, j)
            assert got.dtype == np.float32 and _bits(got)[0, 0] == (ONE if q > 0 else 0), (q, n, j)
    # opposite distances of equal size half way: the zero crossing
    assert kref.merge(np.array([[9]]), np.array([[-9]]), 2, 1)[0, 0] == np.float32(0.5)
    assert kref.merge(np.array([[4]]), np.array([[-1]]), 3, 1)[0, 0] == np.float32(1.0)      # (2 * 2 - 1) / 3 = 1: clamped
    want = np.float64(0.5) + (np.float64(2) * np.sqrt(np.float64(2)) + np.float64(1) * np.float64(-3)) / np.float64(3)
    assert kref.merge(np.array([[2]]), np.array([[-9]]), 3, 1)[0, 0] == np.float32(want) and 0 < want < 1
    # the cap: an empty frame counts as 64 pixels of nothing, whatever the other side's depth
    assert kref.merge(np.array([[far]]), np.array([[-far]]), 2, 1)[0, 0] == np.float32(0.5)
    assert kref.merge(np.array([[100]]), np.array([[-far]]), 8, 1)[0, 0] == np.float32(1.0)  # 0.5 + (7 * 10 - 64) / 8 = 1.25
    assert kref.merge(np.array([[25]]), np.array([[-far]]), 8, 1)[0, 0] == np.float32(0.0)   # 0.5 + (7 * 5 - 64) / 8 < 0
    assert kref.merge(np.array([[4097]]), np.array([[-4097]]), 2, 1)[0, 0] == np.float32(0.5)    # both capped at 64


def test_one_key_is_the_single_key_propagate_and_key_frames_return_their_masks():
    rng = np.random.default_rng(11)
    F, H, W = 5, 23, 33
    video = rng.random((F, H, W, 3), dtype=np.float32)
    soft = rng.random((3, H, W), dtype=np.float32)
    for key in (0, 2, 4):
        got = kref.propagate_keys_ref(video, soft[0], [key], 3, 2, 8)
        assert (_bits(got) == _bits(ref.propagate_ref(video, soft[0], key, 3, 2, 8))).all(), key
    keys = [1, 3]
    got = kref.propagate_keys_ref(video, soft[:2], keys, 3, 2, 8)
    for i, k in enumerate(keys):
        assert (_bits(got[k]) == _bits(ref.binarise(soft[i]).astype(np.float32))).all()
    per_frame = np.zeros((F, H, W), np.float32)
    per_frame[keys] = soft[:2]                                        # [F, H, W]: the frames at the keys are read
    assert (_bits(kref.propagate_keys_ref(video, per_frame, keys, 3, 2, 8)) == _bits(got)).all()
    # outside the keys: the single-key chain of that key alone
    assert (_bits(got[0]) == _bits(ref.propagate_ref(video, soft[0], 1, 3, 2, 8)[0])).all()
    assert (_bits(got[4]) == _bits(ref.propagate_ref(video, soft[1], 3, 3, 2, 8)[4])).all()
    assert got.dtype == np.float32 and (got >= 0).all() and (got <= 1).all()


def test_still_video_empty_and_full():
    rng = np.random.default_rng(12)
    F, H, W = 6, 23, 33
    video = rng.random((F, H, W, 3), dtype=np.float32)
    still = np.repeat(video[:1], F, axis=0)
    soft = rng.random((H, W), dtype=np.float32)
    binar = ref.binarise(soft).astype(np.float32)
    for keys in ([0, 5], [1, 4], [0, 2, 5]):
        got = kref.propagate_keys_ref(still, np.repeat(soft[None], len(keys), axis=0), keys, 3, 2, 8)
        assert (_bits(got) == _bits(np.repeat(binar[None], F, axis=0))).all(), keys
        zeros, ones = np.zeros((len(keys), H, W), np.float32), np.ones((len(keys), H, W), np.float32)
        assert (_bits(kref.propagate_keys_ref(video, zeros, keys, 3, 2, 8)) == 0).all(), keys
        assert (_bits(kref.propagate_keys_ref(video, ones, keys, 3, 2, 8)) == ONE).all(), keys


def test_an_empty_key_next_to_a_painted_one_says_nothing_here():
    """The cap of 64 outweighs a small object's depth: with a 9 x 9 square on key 0 (depth 5) and an empty key 8 the square is
    there while (8 - j) * 5 > j * 64 at its centre, that is on frame j = 0 only; and the mirror image at the other end."""
    F, H, W = 9, 24, 24
    still = np.full((F, H, W, 1), 0.25, np.float32)
    sq = np.zeros((H, W), np.float32)
    sq[8:17, 8:17] = 1
    got = kref.propagate_keys_ref(still, np.stack([sq, np.zeros_like(sq)]), [0, 8], 2, 1, 0)
    assert (got[0] == sq).all() and not got[1:].any()
    got = kref.propagate_keys_ref(still, np.stack([np.zeros_like(sq), sq]), [0, 8], 2, 1, 0)
    assert (got[8] == sq).all() and not got[:8].any()


@functools.lru_cache(maxsize=None)
def _shift_case(shift):
    F, H, W = 5, 96, 112
    big = (np.round(texture((7, 9)) * 255) / 255).astype(np.float32)
    images = np.stack([big[40 - shift[0] * t: 40 - shift[0] * t + H, 40 - shift[1] * t: 40 - shift[1] * t + W] for t in range(F)])
    mask = np.zeros((H, W), np.float32)
    mask[36:60, 40:70] = 1
    truth = np.stack([np.roll(mask, (shift[0] * t, shift[1] * t), (0, 1)) for t in range(F)])
    return kref.luma_pyramids(images[..., None], 3), images[..., None], truth


@functools.lru_cache(maxsize=None)
def _shift_chain(shift, k, d):
    """The longest chain from key k in direction d, painted with the truly shifted mask; shorter chains are its beginning."""
    pyr, _, truth = _shift_case(shift)
    return kref.run_chain(pyr, ref.binarise(truth[k]), k, d, k if d < 0 else 4 - k, 3, 2, 8)


@pytest.mark.parametrize("shift", [(2, -1), (-3, 5)], ids=str)
def test_whole_pixel_shifts_are_tracked_exactly_between_keys(shift):
    _, images, truth = _shift_case(shift)
    for keys in ([0, 4], [0, 2, 4], [1, 3]):
        chain = lambda i, k, d, length: {t: m for t, m in _shift_chain(shift, k, d).items() if abs(t - k) <= length}    # noqa: E731
        out = kref.propagate_keys_ref(images, truth[keys], keys, 3, 2, 8, chain=chain)
        for t in range(5):
            assert (_bits(out[t]) == _bits(truth[t])).all(), (keys, t)


@pytest.mark.parametrize("name", list(SCENES))
def test_the_merge_beats_the_single_key_chain_on_a_moving_disc(name):
    """The quality condition: keys on the first and the last frame, painted with the true discs.  At every frame the merged IoU
    is at least the smaller of the two chains'; over all frames its minimum exceeds the single-key chain's IoU at its last
    frame.  (slow 0.912 against 0.870, still background 0.910 against 0.866, fast 0.925 against 0.875.)"""
    images, discs = disc_scene(*SCENES[name])
    F = len(discs)
    pyr = kref.luma_pyramids(images, 3)
    fwd = kref.run_chain(pyr, discs[0].astype(np.uint8), 0, 1, F - 1, 3, 2, 8)        # its last step is the single-key chain's
    bwd = kref.run_chain(pyr, discs[-1].astype(np.uint8), F - 1, -1, F - 2, 3, 2, 8)
    chain = lambda i, k, d, length: {t: m for t, m in (fwd if d > 0 else bwd).items() if abs(t - k) <= length}    # noqa: E731
    parts = {}
    out = kref.propagate_keys_ref(images, discs[[0, F - 1]].astype(np.float32), [0, F - 1], 3, 2, 8, chain=chain, parts=parts)
    single = _iou(fwd[F - 1] >= 0.5, discs[-1])
    merged = [_iou(out[t] >= 0.5, discs[t]) for t in range(F)]
    for t in range(1, F - 1):
        a, b = _iou(parts[t][0] >= 0.5, discs[t]), _iou(parts[t][1] >= 0.5, discs[t])
        print(name, "frame", t, "merged", round(merged[t], 4), "forward", round(a, 4), "backward", round(b, 4))
        assert merged[t] >= min(a, b), (t, merged[t], a, b)
    print(name, "merged minimum", round(min(merged), 4), "single-key last frame", round(single, 4))
    assert merged[0] == merged[-1] == 1.0
    assert min(merged) > single


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def _jobs(cls, rows):
    arr = (cls * len(rows))(*[cls(*r) for r in rows])
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def test_batched_entries_reject_bad_arguments_without_a_device(hip_lib):
    C, E, U = ctypes, _cabi.LP_E_INVALID, _cabi.LP_E_UNSUPPORTED
    side, grid, J = _cabi.LP_VMASK_MAX_SIDE, _cabi.LP_PROP_MAX_GRID, _cabi.LP_PROP_MAX_JOBS
    assert J == 32
    a = [256 * (i + 1) for i in range(8)]                             # never dereferenced: validation comes before any HIP call

    # match: the descriptor's ranges, then every job's pointers
    good_job = (a[0], a[1], a[2], a[3], a[4], a[5])
    keep, ptr = _jobs(_cabi.LpPropMatchJob, [good_job] * J)
    good = dict(height=40, width=70, levels=3, level=1, search=2, smooth=8, jobs=2, job=ptr)
    assert hip_lib.lp_prop_match_batch(None, None) == E
    for change in ({"height": 0}, {"width": side + 1}, {"levels": 0}, {"levels": 7}, {"level": -1}, {"level": 3}, {"search": 0},
                   {"search": 8}, {"smooth": -1}, {"smooth": 65}, {"jobs": 0}, {"jobs": -1}, {"jobs": J + 1}, {"job": None},
                   {"level": 2}):                                     # the top level with parents given
        assert hip_lib.lp_prop_match_batch(C.byref(_cabi.LpPropMatchBatchDesc(**{**good, **change})), None) == E, change
    for at in (0, 1, J - 1):                                          # one bad job anywhere in the table
        for field, value in (("src", None), ("tgt", None), ("mask", None), ("vec", None), ("valid", None), ("parent", None),
                             ("parent", a[4])):
            rows = [list(good_job) for _ in range(J)]
            rows[at][[f for f, _ in _cabi.LpPropMatchJob._fields_].index(field)] = value
            keep2, ptr2 = _jobs(_cabi.LpPropMatchJob, rows)
            d = _cabi.LpPropMatchBatchDesc(**{**good, "jobs": at + 1, "job": ptr2})
            assert hip_lib.lp_prop_match_batch(C.byref(d), None) == E, (at, field)
    top = [(a[0], a[1], a[2], None, a[4], a[5]), good_job]           # the top level: one job with a parent among those without
    keep3, ptr3 = _jobs(_cabi.LpPropMatchJob, top)
    assert hip_lib.lp_prop_match_batch(C.byref(_cabi.LpPropMatchBatchDesc(**{**good, "level": 2, "job": ptr3})), None) == E

    # fill
    good_job = (a[0], a[1], a[2])
    keep, ptr = _jobs(_cabi.LpPropFillJob, [good_job] * J)
    for bad in ((None, 2, 4, 4), (ptr, 0, 4, 4), (ptr, -3, 4, 4), (ptr, J + 1, 4, 4), (ptr, 2, 0, 4), (ptr, 2, 4, 0),
                (ptr, 2, grid + 1, 4), (ptr, 2, 4, grid + 1)):
        assert hip_lib.lp_prop_fill_batch(*bad, None) == E, bad[1:]
    for at in (0, 3, J - 1):
        for row in ((None, a[1], a[2]), (a[0], None, a[2]), (a[0], a[1], None), (a[0], a[1], a[0])):
            rows = [good_job] * at + [row]
            keep2, ptr2 = _jobs(_cabi.LpPropFillJob, rows)
            assert hip_lib.lp_prop_fill_batch(ptr2, at + 1, 4, 4, None) == E, (at, row)

    # advance: a null pos_src is P_key and is allowed
    good_job = (a[0], a[1], a[2], a[3], a[4], a[5])
    keep, ptr = _jobs(_cabi.LpPropAdvanceJob, [good_job] * J)
    good = dict(height=40, width=70, levels=3, jobs=2, job=ptr)
    assert hip_lib.lp_prop_advance_batch(None, None) == E
    for change in ({"height": 0}, {"height": side + 1}, {"width": 0}, {"levels": 0}, {"levels": 7}, {"jobs": 0}, {"jobs": J + 1},
                   {"job": None}):
        assert hip_lib.lp_prop_advance_batch(C.byref(_cabi.LpPropAdvanceBatchDesc(**{**good, **change})), None) == E, change
    names = [f for f, _ in _cabi.LpPropAdvanceJob._fields_]
    for at in (0, 1, J - 1):
        for field, value in (("vec", None), ("key", None), ("pos_dst", None), ("out", None), ("mask_pyramid", None),
                             ("pos_dst", a[1]), ("mask_pyramid", a[2])):
            rows = [list(good_job) for _ in range(J)]
            rows[at][names.index(field)] = value
            keep2, ptr2 = _jobs(_cabi.LpPropAdvanceJob, rows)
            d = _cabi.LpPropAdvanceBatchDesc(**{**good, "jobs": at + 1, "job": ptr2})
            assert hip_lib.lp_prop_advance_batch(C.byref(d), None) == E, (at, field)

    # merge
    p, q, r = C.c_void_p(256), C.c_void_p(512), C.c_void_p(1024)
    good = dict(frames=3, height=40, width=70, span=7, first=2, qa=p, qb=q, out=r)
    assert hip_lib.lp_prop_merge(None, None) == E
    for change in ({"qa": None}, {"qb": None}, {"out": None}, {"height": 0}, {"height": side + 1}, {"width": 0}, {"width": side + 1},
                   {"span": 1}, {"span": 0}, {"first": 0}, {"first": -1}, {"frames": 0}, {"frames": -1}, {"frames": 6}, {"first": 5},
                   {"out": p}, {"out": q}, {"span": 65536, "first": 65535, "frames": 2}):
        assert hip_lib.lp_prop_merge(C.byref(_cabi.LpPropMergeDesc(**{**good, **change})), None) == E, change
    assert hip_lib.lp_prop_merge(C.byref(_cabi.LpPropMergeDesc(**{**good, "span": 65536})), None) == U
    assert hip_lib.lp_prop_merge(C.byref(_cabi.LpPropMergeDesc(**{**good, "span": 1 << 30, "first": 1 << 29})), None) == U


def test_the_header_says_the_batched_words():
    header = open(os.path.join(ROOT, "include", "lanpaint_hip.h")).read()
    for word in ("LP_PROP_MAX_JOBS", "no FMA", "since |s| >= 1", "This is deliberate", "the caller's error", "Not handled: occlusion."):
        assert word in header, word
    assert "re-anchoring against drift" not in header


# ---- the wrappers and the node ----------------------------------------------------------------------------------------------------------
def test_propagate_keys_refuses_cpu_tensors_and_bad_arguments():
    from lanpaint_amd import propagate_keys as pk
    images, masks = torch.zeros(7, 16, 16, 3), torch.zeros(2, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pk.propagate_keys(images, masks, [0, 6])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pk.propagate_keys(images.numpy(), masks, [0, 6])
    row = torch.zeros(_cabi.prop_pyramid_ws_bytes(1, 16, 16, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pk.match_level_batch([(row, row, row, None)], 16, 16, 3, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pk.fill_median_batch([(torch.zeros(2, 2, 2, dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int32))])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pk.advance_batch([(torch.zeros(2, 2, 2, dtype=torch.int32), None, torch.zeros(16, 16, dtype=torch.uint8))], 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pk.merge_gap(torch.zeros(1, 4, 4, dtype=torch.int32), torch.zeros(1, 4, 4, dtype=torch.int32), 2)
    # the numbers are checked before the tensors are looked at
    for bad in (dict(levels=0), dict(levels=7), dict(levels=2.0), dict(search=0), dict(search=8), dict(smooth=-1), dict(smooth=65),
                dict(smooth=None)):
        with pytest.raises(ValueError):
            pk.propagate_keys(images, masks, [0, 6], **bad)
    for keys in ([], [6, 0], [0, 0], [0, 7], [-1, 3], [0.0, 6], ["0", "6"], [True, 6], None, 3):
        with pytest.raises(ValueError):
            pk.propagate_keys(images, masks, keys)
    for bad in (dict(span=1), dict(span=65536), dict(span=4, first=0), dict(span=4, first=4)):
        with pytest.raises(ValueError):
            pk.merge_gap(torch.zeros(1, 4, 4, dtype=torch.int32), torch.zeros(1, 4, 4, dtype=torch.int32), **bad)
    assert pk.WS_CAP_BYTES == 1 << 30 and pk.MAX_JOBS == 32
    from lanpaint_amd import propagate_keys_nodes
    for module in (pk, propagate_keys_nodes):
        assert sum(1 for _ in open(module.__file__)) <= 900


def test_propagate_keys_node_protocol_and_own_mappings():
    from lanpaint_amd import propagate_keys_nodes, propagate_nodes
    node = propagate_keys_nodes.LanPaint_VideoMaskPropagateKeys
    assert propagate_keys_nodes.NODE_CLASS_MAPPINGS == {"LanPaint_VideoMaskPropagateKeys": node}
    assert list(propagate_keys_nodes.NODE_DISPLAY_NAME_MAPPINGS) == ["LanPaint_VideoMaskPropagateKeys"]
    assert propagate_nodes.NODE_CLASS_MAPPINGS == {"LanPaint_VideoMaskPropagate": propagate_nodes.LanPaint_VideoMaskPropagate}
    types = node.INPUT_TYPES()
    req = types["required"]
    assert list(types) == ["required"] and list(req) == ["image", "mask", "key_frames", "levels", "search", "smooth"]
    assert req["image"][0] == "IMAGE" and req["mask"][0] == "MASK"
    assert req["key_frames"][0] == "STRING" and req["key_frames"][1]["default"] == "0"
    assert req["levels"][0] == "INT" and req["levels"][1] == {**req["levels"][1], "default": 4, "min": 1, "max": 6}
    assert req["search"][0] == "INT" and req["search"][1] == {**req["search"][1], "default": 2, "min": 1, "max": 7}
    assert req["smooth"][0] == "INT" and req["smooth"][1] == {**req["smooth"][1], "default": 8, "min": 0, "max": 64}
    for name in req:
        assert len(req[name][1]["tooltip"]) > 20, name
    for word in ("key frames", "motion", "merged", "stabilize", "mask refine", "encode", "Detailer", "Occlusion", "empty key"):
        assert word in node.DESCRIPTION, word
    assert node.RETURN_TYPES == ("MASK",) and node.FUNCTION == "propagate" and node.CATEGORY == "mask"
    parse = propagate_keys_nodes.parse_key_frames
    assert parse("0") == [0] and parse("0,6") == [0, 6] and parse(" 0 , 3  6,\t9 ") == [0, 3, 6, 9] and parse("3 1") == [3, 1]
    assert parse("") == [] and parse("+2, -1") == [2, -1]
    for bad in ("a", "0;6", "1.5", "0, x", "0x10", None, 3):
        with pytest.raises(ValueError):
            parse(bad)
    images, masks = torch.zeros(7, 16, 16, 3), torch.zeros(2, 16, 16)
    for bad in ("", "6 0", "0 0", "0 7", "-1", "zero"):               # refused before any device is looked for
        with pytest.raises(ValueError):
            node().propagate(images, masks, bad)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            node().propagate(images, masks, "0, 6", 4, 2, 8)
