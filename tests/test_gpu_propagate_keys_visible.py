"""The occlusion-aware video mask propagate from several keyframes on the MI355X (lanpaint_amd.propagate_keys_visible;
lp_prop_visible_batch, lp_prop_occlude_batch and lp_prop_merge_visible in csrc/propagate_kernel.hip) against the numpy restatements
tests/propagate_visible_ref.py and tests/propagate_keys_visible_ref.py.  The rule is integer arithmetic and fp64 in a fixed order, so
every comparison covers every element and has no tolerance.  Each of the three launches is compared on its own, fed with inputs
made here, and the whole call as well.  Without the feature this file fails at its imports."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, propagate, propagate_keys, propagate_keys_visible, propagate_keys_visible_nodes, propagate_visible
from tests import propagate_keys_ref as kref
from tests import propagate_keys_visible_ref as kvref
from tests import propagate_ref as ref
from tests import propagate_visible_ref as vref
from tests.compare import _same_bits, _same_ints as _same
from tests.device import DEV, _dev
from tests.helpers import record_launches
from tests.inputs import VISIBLE_MASKS as MASKS, _counts, _merge_want, _occlude_job, _occluded_video, _rng, _visible_job
from tests.motion_checks import _merge_inputs
from tests.propagate_scenes import occluded_disc_clip

pytestmark = pytest.mark.gpu
# under, at and over the block (8) and the window (16), several 32 x 32 tiles, and widths that are a multiple of 4 (the vector path)
PLANES = [(1, 1), (1, 7), (8, 8), (9, 15), (16, 17), (23, 33), (40, 70), (33, 64), (70, 132)]
LEVELS, SEARCH, SMOOTH = 3, 2, 8
kv = propagate_keys_visible


def _shifted(a):
    """`a` on the device, one element off a 16-byte boundary: a view one element into a larger buffer."""
    buf = torch.empty(a.size + 1, dtype=torch.from_numpy(a[:0]).dtype, device=DEV)
    view = buf[1:].view(a.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return view


# ---- the two batch entries -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jobs", [1, 2, 32])
def test_visible_batch_equals_the_restatement_per_job(jobs):
    for H, W in PLANES:
        for occlusion in (1, 16):
            made = [_visible_job(H, W, j) for j in range(jobs)]
            got = kv.visible_flags_batch([(_dev(P.astype(np.int32)), _dev(Yt), _dev(Yk), _dev(m)) for P, Yt, Yk, m in made], occlusion)
            assert len(got) == jobs
            for j, (P, Yt, Yk, m) in enumerate(made):
                assert got[j].dtype == torch.int32 and tuple(got[j].shape) == ref.grid_of(H, W)
                _same(got[j].cpu().numpy(), vref.visible_flags(Yt, Yk, P, m, occlusion), ("flags", (H, W), jobs, j, occlusion))


@pytest.mark.parametrize("jobs", [1, 2, 32])
def test_occlude_batch_equals_the_restatement_per_job_and_counts_the_visible_bits(jobs):
    for H, W in PLANES:
        made = [_occlude_job(H, W, j) for j in range(jobs)]
        feed = [(_dev((c / 256).astype(np.float32)), _dev(flags.astype(np.int32))) for c, flags in made]
        for levels in (1, 4):
            counts = torch.arange(jobs, dtype=torch.int32, device=DEV) * 3                 # added to, not overwritten
            for with_counts in (True, False):
                got = kv.occlude_batch(feed, levels, counts if with_counts else None)
                for j, (c, flags) in enumerate(made):
                    cv = vref.occlude(c, flags)
                    out, hidden, mpyr = got[j]
                    _same_bits(out.cpu().numpy(), cv.astype(np.float32) / np.float32(256), ("mask", (H, W), jobs, j))
                    _same_bits(hidden.cpu().numpy(), (c - cv).astype(np.float32) / np.float32(256), ("hidden", (H, W), jobs, j))
                    want = ref.pyramid((cv >= 128).astype(np.uint8), levels, ref.down_mask)
                    host = mpyr.cpu()
                    for lv in range(levels):
                        _same(propagate.level_view(host, H, W, lv).numpy()[0], want[lv], ("next bits", (H, W), jobs, j, lv))
            _same(counts.cpu().numpy(), [3 * j + int((vref.occlude(c, flags) >= 128).sum()) for j, (c, flags) in enumerate(made)],
                  ("counts", (H, W), jobs, levels))


def test_a_job_off_16_byte_alignment_takes_the_scalar_path_next_to_one_that_does_not():
    H, W = 33, 64
    made = [_visible_job(H, W, j) for j in range(2)]
    feed = [(_dev(made[0][0].astype(np.int32)), _dev(made[0][1]), _dev(made[0][2]), _dev(made[0][3])),
            (_shifted(made[1][0].astype(np.int32)), _shifted(made[1][1]), _dev(made[1][2]), _shifted(made[1][3]))]
    got = kv.visible_flags_batch(feed, 16)
    for j, (P, Yt, Yk, m) in enumerate(made):
        _same(got[j].cpu().numpy(), vref.visible_flags(Yt, Yk, P, m, 16), ("flags", j))
    made = [_occlude_job(H, W, j) for j in range(2)]
    counts = torch.zeros(2, dtype=torch.int32, device=DEV)
    got = kv.occlude_batch([(_dev((made[0][0] / 256).astype(np.float32)), _dev(made[0][1].astype(np.int32))),
                            (_shifted((made[1][0] / 256).astype(np.float32)), _dev(made[1][1].astype(np.int32)))], 3, counts)
    for j, (c, flags) in enumerate(made):
        cv = vref.occlude(c, flags)
        _same_bits(got[j][0].cpu().numpy(), cv.astype(np.float32) / np.float32(256), ("mask", j))
        _same_bits(got[j][1].cpu().numpy(), (c - cv).astype(np.float32) / np.float32(256), ("hidden", j))
        assert int(counts[j]) == int((cv >= 128).sum())


def test_jobs_outside_1_to_32_are_invalid():
    lib, H, W = _cabi.load(), 9, 15
    P, Yt, Yk, m = _visible_job(H, W, 0)
    keep = [_dev(P.astype(np.int32)), _dev(Yt), _dev(Yk), _dev(m), torch.empty(ref.grid_of(H, W), dtype=torch.int32, device=DEV)]
    table = np.array([[t.data_ptr() for t in keep]] * 33, dtype=np.uint64)
    c, flags = _occlude_job(H, W, 0)
    keep2 = [_dev((c / 256).astype(np.float32)), _dev(flags.astype(np.int32)), torch.empty((H, W), device=DEV), torch.empty((H, W), device=DEV),
             torch.empty(_cabi.prop_pyramid_ws_bytes(1, H, W, 3), dtype=torch.uint8, device=DEV)]
    table2 = np.array([[t.data_ptr() for t in keep2] + [0]] * 33, dtype=np.uint64)
    for jobs in (0, 33, -1):
        d = _cabi.LpPropVisibleBatchDesc(H, W, 16, jobs, table.ctypes.data)
        assert lib.lp_prop_visible_batch(ctypes.byref(d), None) == _cabi.LP_E_INVALID
        d = _cabi.LpPropOccludeBatchDesc(H, W, 3, jobs, table2.ctypes.data)
        assert lib.lp_prop_occlude_batch(ctypes.byref(d), None) == _cabi.LP_E_INVALID
    with pytest.raises(ValueError):
        kv.visible_flags_batch([tuple(keep[:4])] * 33, 16)
    with pytest.raises(ValueError):
        kv.occlude_batch([tuple(keep2[:2])] * 33, 3)


# ---- the merge ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plane", [(1, 1), (9, 15), (23, 33), (70, 132)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("span", [2, 3, 7])
def test_merge_visible_equals_the_restatement(plane, span):
    H, W = plane
    seen = set()
    for flag_kind in ("none", "all", "random"):
        q, c, cv, f = _merge_inputs(H, W, span, flag_kind)
        dq, dc, dcv, df = (_dev(q.astype(np.int32)), _dev((c / 256).astype(np.float32)), _dev((cv / 256).astype(np.float32)),
                           _dev(f.astype(np.int32)))
        for kind in ("none_lost", "a_lost", "b_lost", "both_lost", "small_key"):
            na, nb = _counts(kind, span)
            want, want_hidden = _merge_want(q, c, cv, f, na, nb, span)
            seen.update((kvref.lost_at(na, j), kvref.lost_at(nb, span - j)) for j in range(1, span))
            dna, dnb = _dev(np.array(na, np.int32)), _dev(np.array(nb, np.int32))
            out, hidden = kv.merge_gap_visible(dq[0], dq[1], dc[0], dcv[0], dc[1], dcv[1], df[0], df[1], dna, dnb, span)
            _same_bits(out.cpu().numpy(), want, ("mask", plane, span, flag_kind, kind))
            _same_bits(hidden.cpu().numpy(), want_hidden, ("hidden", plane, span, flag_kind, kind))
            # the chunked form: one frame per launch through `first`; and in place on the forward chain's planes
            for i in range(span - 1):
                o, h = kv.merge_gap_visible(dq[0, i:i + 1], dq[1, i:i + 1], dc[0, i:i + 1], dcv[0, i:i + 1], dc[1, i:i + 1], dcv[1, i:i + 1],
                                            df[0, i:i + 1], df[1, i:i + 1], dna, dnb, span, i + 1)
                _same_bits(o.cpu().numpy(), want[i:i + 1], ("mask, first", plane, span, flag_kind, kind, i))
                _same_bits(h.cpu().numpy(), want_hidden[i:i + 1], ("hidden, first", plane, span, flag_kind, kind, i))
            code_a, mask_a = dc[0].clone(), dcv[0].clone()
            kv.merge_gap_visible(dq[0], dq[1], code_a, mask_a, dc[1], dcv[1], df[0], df[1], dna, dnb, span, 1, mask_a, code_a)
            assert torch.equal(mask_a, out) and torch.equal(code_a, hidden)
    assert seen == {(False, False), (True, False), (False, True), (True, True)}


def test_merge_visible_off_16_byte_alignment_takes_the_scalar_path_with_the_same_bits():
    H, W, span = 33, 64, 3
    q, c, cv, f = _merge_inputs(H, W, span, "random")
    na, nb = _counts("a_lost", span)
    want, want_hidden = _merge_want(q, c, cv, f, na, nb, span)
    code = [(c[x] / 256).astype(np.float32) for x in range(2)]
    out, hidden = kv.merge_gap_visible(_dev(q[0].astype(np.int32)), _shifted(q[1].astype(np.int32)), _shifted(code[0]), _dev((cv[0] / 256).astype(np.float32)),
                                       _dev(code[1]), _dev((cv[1] / 256).astype(np.float32)), _dev(f[0].astype(np.int32)), _dev(f[1].astype(np.int32)),
                                       _dev(np.array(na, np.int32)), _dev(np.array(nb, np.int32)), span)
    _same_bits(out.cpu().numpy(), want, "mask")
    _same_bits(hidden.cpu().numpy(), want_hidden, "hidden")


# ---- the whole call --------------------------------------------------------------------------------------------------------------------
def _painted(mask, keys):
    """A painting per key: the video's disc, moved along by the key's number so that the keys differ."""
    return np.stack([np.roll(mask, (k, -2 * k), (0, 1)) for k in keys])


@functools.lru_cache(maxsize=None)
def _want(F, H, W, keys, occlusion=16):
    images, mask = _occluded_video(F, H, W)
    trace = {}
    return kvref.propagate_keys_visible_ref(images, _painted(mask, keys), list(keys), LEVELS, SEARCH, SMOOTH, occlusion, trace), trace


KEY_SETS = {1: [(0,)], 2: [(1,), (0, 1)], 3: [(1,), (0, 2), (0, 1, 2)], 7: [(3,), (0, 6), (0, 3, 6), (2, 3), (1, 5)],
            9: [(0, 8), (0, 4, 8), (4, 5), (1, 7), (2, 3, 7)]}


@pytest.mark.parametrize("plane", [(23, 33), (70, 130)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("frames", [1, 2, 3, 7, 9])
def test_the_whole_call_equals_the_restatement_bit_for_bit(plane, frames):
    H, W = plane
    images, mask = _occluded_video(frames, H, W)
    t = _dev(images)
    for keys in KEY_SETS[frames]:
        (want, want_hidden), _ = _want(frames, H, W, keys)
        masks = _painted(mask, keys)
        got, hidden = kv.propagate_keys_visible(t, _dev(masks), list(keys), LEVELS, SEARCH, SMOOTH)              # the default occlusion
        assert got.is_cuda and hidden.is_cuda and got.dtype == hidden.dtype == torch.float32
        _same_bits(got.cpu().numpy(), want, ("mask", plane, frames, keys))
        _same_bits(hidden.cpu().numpy(), want_hidden, ("hidden", plane, frames, keys))
        for i, k in enumerate(keys):                                  # on every key the painting
            _same_bits(want[k], ref.binarise(masks[i]).astype(np.float32), "a key frame is its binarised mask")
            assert not want_hidden[k].any()
        total = (want.astype(np.float64) + want_hidden) * 256
        assert (total == np.round(total)).all()
        if len(keys) < frames:                                        # [F, H, W]: what is not on a key frame is not read
            per_frame = np.full((frames, H, W), 0.75, np.float32)
            per_frame[list(keys)] = masks
            again, again_hidden = kv.propagate_keys_visible(t, _dev(per_frame), list(keys), LEVELS, SEARCH, SMOOTH, 16)
            assert torch.equal(again, got) and torch.equal(again_hidden, hidden)
    if frames == 9 and plane == (70, 130):                            # the occluder is seen
        assert _want(9, H, W, (0, 8))[0][1].sum() > 0


@functools.lru_cache(maxsize=None)
def _quality():
    images, discs, _ = occluded_disc_clip(seed=0, F=16, H=64, W=96, radius=12, bar=(28, 44))
    masks = np.stack([discs[0], discs[15]]).astype(np.float32)
    trace = {}
    return images, masks, kvref.propagate_keys_visible_ref(images, masks, [0, 15], LEVELS, SEARCH, SMOOTH, 16, trace), trace


def test_the_clip_on_which_chains_get_lost():
    images, masks, (want, want_hidden), trace = _quality()
    lost = trace["lost"]
    assert {lost[t] for t in lost} >= {(False, True), (True, False)}   # either chain is lost somewhere, and exactly one on some frame
    got, hidden = kv.propagate_keys_visible(_dev(images), _dev(masks), [0, 15], LEVELS, SEARCH, SMOOTH, 16)
    _same_bits(got.cpu().numpy(), want, "mask")
    _same_bits(hidden.cpu().numpy(), want_hidden, "hidden")
    again, again_hidden = kv.propagate_keys_visible(_dev(images), _dev(masks), [0, 15], LEVELS, SEARCH, SMOOTH, 16)
    assert torch.equal(again, got) and torch.equal(again_hidden, hidden)                                     # two runs, the same bits


STEP = ["lp_prop_match_batch", "lp_prop_fill_batch"] * LEVELS + ["lp_prop_advance_batch", "lp_prop_visible_batch", "lp_prop_occlude_batch"]


def test_more_chains_than_one_launch_holds(monkeypatch):
    """A key on every even frame of 40: 19 gaps of one frame and the last frame, 39 chains of one step, so every stage of the step
    takes two launches (32 + 7), and so does the count of the 38 gap chains' key bits."""
    F, H, W = 40, 9, 15
    keys = list(range(0, F, 2))
    assert len(propagate_keys.chain_plan(F, keys)) == 39
    images = _rng(F, H, W, 41).random((F, H, W, 3), dtype=np.float32)
    masks = np.stack([MASKS[("disc", "full", "sparse")[k % 3]](H, W).astype(np.float32) for k in keys])
    names = record_launches(monkeypatch, propagate_keys, propagate_keys_visible)
    got, hidden = kv.propagate_keys_visible(_dev(images), _dev(masks), keys, LEVELS, SEARCH, SMOOTH, 16)
    batched = [n for n in names if n.endswith("_batch")]
    assert batched == ["lp_prop_occlude_batch"] * 2 + STEP * 2 and names.count("lp_prop_merge_visible") == 19
    want, want_hidden = kvref.propagate_keys_visible_ref(images, masks, keys, LEVELS, SEARCH, SMOOTH, 16)
    _same_bits(got.cpu().numpy(), want, "39 chains")
    _same_bits(hidden.cpu().numpy(), want_hidden, "39 chains")


def test_the_active_chains_are_no_prefix_of_the_plan_and_more_than_one_launch_holds(monkeypatch):
    """Keys on 0, 2, ..., 64 and on 69 of 70 frames: 64 chains of one step, then the two chains of the gap 64 to 69 with four.  Step
    1 takes three launches per stage (32 + 32 + 2 jobs), as does the count of the 66 chains' key bits; steps 2 to 4 run plan rows 64
    and 65 alone, in the field walk's scratch rows 0 and 1."""
    F, H, W = 70, 9, 15
    keys = list(range(0, 65, 2)) + [69]
    plan = propagate_keys.chain_plan(F, keys)
    assert len(plan) == 66 and [c[3] for c in plan] == [1] * 64 + [4, 4]
    images = _rng(F, H, W, 43).random((F, H, W, 3), dtype=np.float32)
    masks = np.stack([MASKS[("disc", "full", "sparse")[k % 3]](H, W).astype(np.float32) for k in keys])
    names = record_launches(monkeypatch, propagate_keys, propagate_keys_visible)
    got, hidden = kv.propagate_keys_visible(_dev(images), _dev(masks), keys, LEVELS, SEARCH, SMOOTH, 16)
    batched = [n for n in names if n.endswith("_batch")]
    assert batched == ["lp_prop_occlude_batch"] * 3 + STEP * (3 + 3) and names.count("lp_prop_merge_visible") == 33
    want, want_hidden = kvref.propagate_keys_visible_ref(images, masks, keys, LEVELS, SEARCH, SMOOTH, 16)
    _same_bits(got.cpu().numpy(), want, "66 chains")
    _same_bits(hidden.cpu().numpy(), want_hidden, "66 chains")


def test_the_launches_of_a_call_and_the_merge_in_chunks(monkeypatch):
    """F = 7 with keys on both ends: two chains of 5 steps side by side, 2 L + 3 launches per step; one launch counts both keys'
    bits; one merge for the gap, or one per frame when the distances go a frame at a time."""
    H, W = 70, 130
    images, mask = _occluded_video(7, H, W)
    t, m = _dev(images), _dev(_painted(mask, (0, 6)))
    names = record_launches(monkeypatch, propagate_keys, propagate_keys_visible)
    got, hidden = kv.propagate_keys_visible(t, m, [0, 6], LEVELS, SEARCH, SMOOTH, 16)
    batched = [n for n in names if n.endswith("_batch")]
    assert batched == ["lp_prop_occlude_batch"] + STEP * 5
    assert names.count("lp_prop_merge_visible") == 1 and names.count("lp_prop_luma") == 1 and names.count("lp_prop_merge") == 0
    assert not [n for n in names if n in ("lp_prop_match", "lp_prop_fill", "lp_prop_advance", "lp_prop_visible", "lp_prop_occlude")]
    (want, want_hidden), _ = _want(7, H, W, (0, 6))
    _same_bits(got.cpu().numpy(), want, "mask")
    del names[:]
    real = kv.chunks
    monkeypatch.setattr(kv, "chunks", lambda n, per, cap: real(n, per, per))
    again, again_hidden = kv.propagate_keys_visible(t, m, [0, 6], LEVELS, SEARCH, SMOOTH, 16)
    assert names.count("lp_prop_merge_visible") == 5 and torch.equal(again, got) and torch.equal(again_hidden, hidden)
    monkeypatch.undo()
    kept = 5 * 2 * (H * W * 4 + 9 * 17 * 4) + 3 * (H * W * 4 + 9 * 17 * 4)
    monkeypatch.setattr(kv, "WS_CAP_BYTES", kept - 1)
    with pytest.raises(ValueError, match=f"{kept} bytes.*{kept - 1}"):
        kv.propagate_keys_visible(t, m, [0, 6], LEVELS, SEARCH, SMOOTH, 16)
    monkeypatch.setattr(kv, "WS_CAP_BYTES", kept)
    again, again_hidden = kv.propagate_keys_visible(t, m, [0, 6], LEVELS, SEARCH, SMOOTH, 16)
    assert torch.equal(again, got) and torch.equal(again_hidden, hidden)


# ---- what follows from the rule -----------------------------------------------------------------------------------------------------------
def test_one_key_is_propagate_masks_visible():
    H, W = 70, 130
    images, mask = _occluded_video(7, H, W)
    t, m = _dev(images), _dev(mask)
    for key in (0, 3, 6):
        got, hidden = kv.propagate_keys_visible(t, m[None], [key], LEVELS, SEARCH, SMOOTH, 16)
        want, want_hidden = propagate_visible.propagate_masks_visible(t, m, key, LEVELS, SEARCH, SMOOTH, 16)
        assert torch.equal(got, want) and torch.equal(hidden, want_hidden), key
        got, hidden = kv.propagate_keys_visible(t, m, [key], LEVELS, SEARCH, SMOOTH, 16)                      # [H, W] for one key
        assert torch.equal(got, want) and torch.equal(hidden, want_hidden), key


def test_occlusion_zero_is_propagate_keys_and_makes_no_new_launch(monkeypatch):
    H, W = 40, 70
    images, mask = _occluded_video(7, H, W)
    t, m = _dev(images), _dev(_painted(mask, (1, 5)))
    want = propagate_keys.propagate_keys(t, m, [1, 5], LEVELS, SEARCH, SMOOTH)
    names = record_launches(monkeypatch, propagate_keys, propagate_keys_visible)
    got, hidden = kv.propagate_keys_visible(t, m, [1, 5], LEVELS, SEARCH, SMOOTH, 0)
    assert torch.equal(got, want)
    assert hidden.is_cuda and hidden.dtype == torch.float32 and tuple(hidden.shape) == (7, H, W) and not hidden.any()
    assert names and not [n for n in names if n in ("lp_prop_visible_batch", "lp_prop_occlude_batch", "lp_prop_merge_visible")]


def test_a_still_video_and_empty_keys():
    H, W = 40, 70
    images, mask = _occluded_video(7, H, W)
    t = _dev(images)
    soft = _rng(H, W, 51).random((H, W), dtype=np.float32)
    still = t[:1].repeat(7, 1, 1, 1)
    got, hidden = kv.propagate_keys_visible(still, _dev(np.repeat(soft[None], 3, axis=0)), [0, 2, 6], LEVELS, SEARCH, SMOOTH, 1)
    _same_bits(got.cpu().numpy(), np.repeat(ref.binarise(soft).astype(np.float32)[None], 7, axis=0), "a still video")
    assert not hidden.any()
    got, hidden = kv.propagate_keys_visible(t, torch.zeros((3, H, W), device=DEV), [0, 2, 6], LEVELS, SEARCH, SMOOTH, 1)
    assert not got.any() and not hidden.any()
    for bad_masks in (torch.zeros((2, H, W), device=DEV), torch.zeros((3, H, W - 1), device=DEV)):
        with pytest.raises(ValueError):
            kv.propagate_keys_visible(t, bad_masks, [0, 2, 6])
    for bad_keys in ([5, 1], [1, 1], [1, 7], []):
        with pytest.raises(ValueError):
            kv.propagate_keys_visible(t, torch.zeros((2, H, W), device=DEV), bad_keys)


def test_node_returns_what_the_module_returns_on_the_inputs_device():
    H, W = 23, 33
    images, mask = _occluded_video(7, H, W)
    masks = _painted(mask, (0, 3, 6))
    node = propagate_keys_visible_nodes.LanPaint_VideoMaskPropagateKeysVisible()
    (want, want_hidden), _ = _want(7, H, W, (0, 3, 6))
    out, hidden = node.propagate(torch.from_numpy(images), torch.from_numpy(masks), "0, 3 6", LEVELS, SEARCH, SMOOTH, 16)
    assert not out.is_cuda and not hidden.is_cuda and out.dtype == hidden.dtype == torch.float32
    _same_bits(out.numpy(), want, "host in, host out")
    _same_bits(hidden.numpy(), want_hidden, "host in, host out")
    on_i, on_m = _dev(images), _dev(masks)
    out, hidden = node.propagate(on_i, on_m, "0,3,6", LEVELS, SEARCH, SMOOTH, 16)
    m, h = kv.propagate_keys_visible(on_i, on_m, [0, 3, 6], LEVELS, SEARCH, SMOOTH, 16)
    assert out.device == hidden.device == on_m.device and torch.equal(out, m) and torch.equal(hidden, h)
    out, hidden = node.propagate(on_i, on_m[:1])                      # the defaults: key 0, levels 4, search 2, smooth 8, occlusion 16
    m, h = propagate_visible.propagate_masks_visible(on_i, on_m[0], 0, 4, 2, 8, 16)
    assert torch.equal(out, m) and torch.equal(hidden, h)
