"""The anchored video mask propagate from several keyframes on the MI355X (lanpaint_amd.propagate_keys_anchored; the warped-key
form of lp_prop_match_batch, lp_prop_anchor_match_kernel in csrc/propagate_kernel.hip) against the numpy restatements
tests/propagate_keys_anchored_ref.py and tests/propagate_anchored_ref.py and against the single entry.  The rule is integer
arithmetic, so every comparison covers every element and has no tolerance.  Without the feature this file fails at its imports."""
import functools
import time

import numpy as np
import pytest
import torch

from lanpaint_amd import (_cabi, propagate, propagate_anchored, propagate_keys, propagate_keys_anchored,
                          propagate_keys_anchored_nodes)
from tests import propagate_keys_anchored_ref as karef
from tests import propagate_keys_ref as kref
from tests import propagate_ref as ref
from tests.compare import _f32_bits as _bits, _same_bits, _same_ints as _same
from tests.device import DELAY_MS, DEV, _dev, _equal, _spin_cycles_per_ms
from tests.helpers import record_launches
from tests.inputs import (BATCH_PLANES, JOB_MASKS, KEYS_ANCHORED_ANCHOR as ANCHOR, KEYS_ANCHORED_CLIPS as CLIPS,
                          KEYS_ANCHORED_LEVELS as LEVELS, KEYS_ANCHORED_SEARCH as SEARCH, KEYS_ANCHORED_SMOOTH as SMOOTH, MASKS, _job,
                          _job_field, _keys_anchored_clip as _clip, _soft, _video)
from tests.motion_checks import _offset_view
from tests.poison import poisoned_empty
from tests.propagate_scenes import assert_the_two_gap_iou_lines as assert_the_two_iou_lines, gap_drift_case

pytestmark = pytest.mark.gpu
ONE = np.float32(1.0).view(np.uint32)
STEP = ["lp_prop_match_batch", "lp_prop_fill_batch"] * LEVELS + ["lp_prop_advance_batch", "lp_prop_match_batch", "lp_prop_fill_batch",
                                                                  "lp_prop_advance_batch"]


# ---- the batched warped match -----------------------------------------------------------------------------------------------------------
NUMBERS = [(1, 0), (2, 8), (7, 64)]                                    # anchor, smooth


@pytest.mark.parametrize("plane", BATCH_PLANES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("jobs", [1, 2, 5, 32])
def test_the_batched_warped_match_equals_the_single_entry_and_the_restatement(plane, jobs, monkeypatch):
    """Odd jobs lie 4 bytes into their buffers: on (40, 72) they take the scalar path and the even ones the vector path, in one
    launch.  The outputs come poisoned, so a cell that nobody writes shows."""
    H, W = plane
    gh, gw = _cabi.prop_grid(H, W)
    for levels, (anchor, smooth) in zip((1, 3, 2), NUMBERS):
        stride = _cabi.prop_pyramid_ws_bytes(1, H, W, levels)
        rows, planes = [], []
        for i in range(jobs):
            P, Yt, Yk, m = _job(H, W, i)
            off = 4 * (i & 1)
            key, tgt, mpyr, pos = _offset_view(Yk, off, stride), _offset_view(Yt, off, stride), _offset_view(m, off, stride), _offset_view(P, off)
            assert all(t.data_ptr() % 16 == off for t in (key, tgt, mpyr, pos))
            rows.append((key, tgt, mpyr, pos))
            planes.append([t[:H * W].view(H, W) for t in (tgt, key, mpyr)])
        filled = poisoned_empty(monkeypatch, 0xFF)
        got = propagate_keys.anchor_field_batch(rows, H, W, levels, anchor, smooth)
        assert len(got) == jobs and len(filled) == 2 * jobs
        monkeypatch.undo()
        for i in range(jobs):
            what = (plane, jobs, "levels", levels, "anchor", anchor, "smooth", smooth, "job", i)
            vec, valid = got[i]
            assert vec.dtype == valid.dtype == torch.int32 and tuple(vec.shape) == (gh, gw, 2) and tuple(valid.shape) == (gh, gw)
            tgt, key, bits = planes[i]
            want_vec, want_valid = propagate_anchored.anchor_field(rows[i][3], tgt, key, bits, anchor, smooth)
            _equal(vec, want_vec, (*what, "vec against lp_prop_anchor_match"))
            _equal(valid, want_valid, (*what, "valid against lp_prop_anchor_match"))
            ref_vec, ref_valid = _job_field(H, W, i, anchor, smooth)
            _same(valid.cpu().numpy(), ref_valid, (*what, "valid"))
            _same(vec.cpu().numpy(), ref_vec, (*what, "vec"))
            if JOB_MASKS[i % len(JOB_MASKS)] in ("15 pixels", "empty"):   # no live block: all zero
                assert int(_job(H, W, i)[3].sum()) == (min(15, H * W) if i % 5 == 2 else 0)
                assert not vec.any() and not valid.any(), what


def test_the_batched_warped_match_moves_and_refuses():
    """What the comparison above rests on: the jobs' fields are not all zero, whole and sub-pixel; and the wrapper's refusals."""
    H, W = 40, 72
    for anchor, smooth in NUMBERS:
        fields = [_job_field(H, W, i, anchor, smooth) for i in range(5)]
        assert any(v.any() for v, _ in fields) and any((v % 16 != 0).any() for v, _ in fields), anchor
        assert any(ok.any() and not ok.all() for _, ok in fields), anchor
    stride = _cabi.prop_pyramid_ws_bytes(1, H, W, 2)
    row = torch.zeros(stride, dtype=torch.uint8, device=DEV)
    pos = torch.zeros((H, W, 2), dtype=torch.int32, device=DEV)
    assert len(propagate_keys.anchor_field_batch([(row, row, row, pos)] * 32, H, W, 2, 1, 0)) == 32
    for bad in ([], [(row, row, row, pos)] * 33, [(row, row, row[:-1], pos)], [(row, row, row, pos[:-1])], [(row, row, row, pos.float())]):
        with pytest.raises(ValueError):
            propagate_keys.anchor_field_batch(bad, H, W, 2, 1, 0)
    for bad in (dict(anchor=0), dict(anchor=8), dict(smooth=65), dict(levels=0)):
        with pytest.raises(ValueError):
            propagate_keys.anchor_field_batch([(row, row, row, pos)], H, W, **{"levels": 2, "anchor": 2, "smooth": 8, **bad})
    # the library itself, on real buffers: an output on an input, or the two outputs on one another
    vec, valid = torch.zeros((5, 9, 2), dtype=torch.int32, device=DEV), torch.zeros((5, 9), dtype=torch.int32, device=DEV)
    lib = _cabi.load()
    for job in ((row, row, row, pos, pos, valid), (row, row, row, pos, vec, vec), (row, row, row, None, vec, valid)):
        table = propagate_keys.job_table([job], "refusals")
        d = _cabi.LpPropMatchBatchDesc(H, W, 2, 0, 2, 8, 1, _cabi.LP_PROP_MATCH_WARPED_KEY, table.ctypes.data)
        assert lib.lp_prop_match_batch(d, None) == _cabi.LP_E_INVALID
    table = propagate_keys.job_table([(row, row, row, pos, vec, valid)], "refusals")
    for form in (2, -1):
        d = _cabi.LpPropMatchBatchDesc(H, W, 2, 0, 2, 8, 1, form, table.ctypes.data)
        assert lib.lp_prop_match_batch(d, None) == _cabi.LP_E_INVALID
    torch.cuda.synchronize()


# ---- the whole call ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _longest_chain(plane, half, k, d):
    """The longest anchored chain from key k in direction d; a shorter chain is its beginning."""
    images, Y, pyr, painted = _clip(plane, half)
    F = len(images)
    return karef.run_chain(pyr, Y, ref.binarise(painted[k]), k, d, k if d < 0 else F - 1 - k, LEVELS, SEARCH, SMOOTH, ANCHOR)


def _want(plane, keys, half=False):
    images, _, _, painted = _clip(plane, half)
    chain = lambda i, k, d, length: {t: m for t, m in _longest_chain(plane, half, k, d).items() if abs(t - k) <= length}    # noqa: E731
    return kref.propagate_keys_ref(images, painted[keys], keys, LEVELS, SEARCH, SMOOTH, chain=chain)


def _run(plane, keys, half=False):
    images, _, _, painted = _clip(plane, half)
    t = _dev(images).half() if half else _dev(images)
    got = propagate_keys_anchored.propagate_keys_anchored(t, _dev(painted[keys]), keys, LEVELS, SEARCH, SMOOTH, ANCHOR)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (len(images), *plane)
    return got


@pytest.mark.parametrize("plane", list(CLIPS), ids=lambda s: "x".join(map(str, s)))
def test_the_whole_call_equals_the_restatement_for_every_key_set(plane):
    H, W = plane
    F, key_sets = CLIPS[plane]
    images, _, _, painted = _clip(plane)
    t = _dev(images)
    for keys in key_sets:
        got, want = _run(plane, keys), _want(plane, keys)
        _same_bits(got.cpu().numpy(), want, (plane, keys))             # 0 differing elements
        for k in keys:
            _same_bits(want[k], ref.binarise(painted[k]).astype(np.float32), "a key frame is its binarised mask")
        masks = [_dev(painted[k]) for k in keys]
        first = propagate_anchored.propagate_masks_anchored(t, masks[0], keys[0], LEVELS, SEARCH, SMOOTH, ANCHOR)
        if len(keys) == 1:                                             # K = 1 is propagate_masks_anchored, and [H, W] is accepted
            _equal(got, first, ("K = 1", plane, keys))
            _equal(propagate_keys_anchored.propagate_keys_anchored(t, masks[0], keys, LEVELS, SEARCH, SMOOTH, ANCHOR), first, "[H, W]")
        else:                                                          # outside the keys: the single-key anchored chain of that key
            last = propagate_anchored.propagate_masks_anchored(t, masks[-1], keys[-1], LEVELS, SEARCH, SMOOTH, ANCHOR)
            _equal(got[:keys[0] + 1], first[:keys[0] + 1], ("in front of the first key", plane, keys))
            _equal(got[keys[-1]:], last[keys[-1]:], ("behind the last key", plane, keys))
            per_frame = np.full((F, H, W), 0.75, np.float32)           # what is not on a key frame is not read
            per_frame[keys] = painted[keys]
            _equal(propagate_keys_anchored.propagate_keys_anchored(t, _dev(per_frame), keys, LEVELS, SEARCH, SMOOTH, ANCHOR), got, "[F, H, W]")
    if plane == (40, 70):                                              # the correction is at work here: not the several-keys bits
        plain = propagate_keys.propagate_keys(t, _dev(painted[[0, 6]]), [0, 6], LEVELS, SEARCH, SMOOTH)
        assert not torch.equal(plain, _run(plane, [0, 6]))


def test_anchor_zero_is_propagate_keys_and_makes_no_new_launch(monkeypatch):
    plane, keys = (40, 70), [0, 3, 6]
    images, _, _, painted = _clip(plane)
    t, m = _dev(images), _dev(painted[keys])
    names = record_launches(monkeypatch, propagate_keys_anchored, propagate_keys)
    want = propagate_keys.propagate_keys(t, m, keys, LEVELS, SEARCH, SMOOTH)
    plain = list(names)
    assert len([n for n in plain if n.endswith("_batch")]) == 2 * (2 * LEVELS + 1)
    del names[:]
    got = propagate_keys_anchored.propagate_keys_anchored(t, m, keys, LEVELS, SEARCH, SMOOTH, 0)
    assert names == plain and torch.equal(got, want)                   # nothing but what propagate_keys launches itself
    del names[:]
    propagate_keys_anchored.propagate_keys_anchored(t, m, keys, LEVELS, SEARCH, SMOOTH, ANCHOR)
    assert [n for n in names if n.endswith("_batch")] == STEP * 2
    assert [n for n in names if not n.endswith("_batch")] == [n for n in plain if not n.endswith("_batch")]


def test_a_still_video_empty_full_and_half_precision_images():
    H, W = 40, 70
    F = 7
    still = _dev(np.repeat(_video(1, H, W), F, axis=0))
    soft = _soft(H, W, 3)
    for anchor in (2, 7):
        got = propagate_keys_anchored.propagate_keys_anchored(still, _dev(np.repeat(soft[None], 3, axis=0)), [0, 2, 6], LEVELS, SEARCH, SMOOTH, anchor)
        _same_bits(got.cpu().numpy(), np.repeat(ref.binarise(soft).astype(np.float32)[None], F, axis=0), ("a still video", anchor))
    moving = _dev(_clip((40, 70))[0])
    for keys in ([0, 6], [1, 4], [0, 3, 6]):
        zeros, ones = torch.zeros((len(keys), H, W), device=DEV), torch.ones((len(keys), H, W), device=DEV)
        got = propagate_keys_anchored.propagate_keys_anchored(moving, zeros, keys, LEVELS, SEARCH, SMOOTH, 7)
        assert (_bits(got.cpu().numpy()) == 0).all(), keys             # exactly 0.0
        got = propagate_keys_anchored.propagate_keys_anchored(moving, ones, keys, LEVELS, SEARCH, SMOOTH, 7)
        assert (_bits(got.cpu().numpy()) == ONE).all(), keys           # exactly 1.0
    for plane, keys in (((9, 7), [0, 2, 5]), ((40, 70), [1, 5])):      # fp16 images: the restatement on the half-rounded values
        _same_bits(_run(plane, keys, half=True).cpu().numpy(), _want(plane, keys, half=True), ("fp16", plane, keys))


def test_more_chains_than_one_launch_holds(monkeypatch):
    """A key on every even frame of 36: 35 chains of one step, so every stage of the step takes two launches (32 + 3)."""
    F, H, W = 36, 24, 40
    keys = list(range(0, F, 2))
    assert len(propagate_keys.chain_plan(F, keys)) == 35
    images = _video(F, H, W, 3, seed=2)
    masks = np.stack([MASKS[("disc", "soft", "full")[k % 3]](H, W, k) for k in keys])
    names = record_launches(monkeypatch, propagate_keys_anchored, propagate_keys)
    got = propagate_keys_anchored.propagate_keys_anchored(_dev(images), _dev(masks), keys, LEVELS, SEARCH, SMOOTH, ANCHOR)
    batched = [n for n in names if n.endswith("_batch")]
    assert batched == STEP * 2 and names.count("lp_prop_merge") == 17
    _same_bits(got.cpu().numpy(), karef.propagate_keys_anchored_ref(images, masks, keys, LEVELS, SEARCH, SMOOTH, ANCHOR), "35 chains")


def test_the_chains_of_a_step_share_their_launches(monkeypatch):
    """F = 7 with keys on both ends at 3 levels: two chains of 5 steps run side by side, exactly 5 x 10 batched launches."""
    plane = (40, 70)
    images, _, _, painted = _clip(plane)
    names = record_launches(monkeypatch, propagate_keys_anchored, propagate_keys)
    propagate_keys_anchored.propagate_keys_anchored(_dev(images), _dev(painted[[0, 6]]), [0, 6], LEVELS, SEARCH, SMOOTH, ANCHOR)
    batched = [n for n in names if n.endswith("_batch")]
    assert len(batched) == 5 * (2 * LEVELS + 4) == 50 and batched == STEP * 5
    assert names.count("lp_prop_merge") == 1 and names.count("lp_prop_luma") == 1
    assert not [n for n in names if n in ("lp_prop_match", "lp_prop_fill", "lp_prop_advance", "lp_prop_anchor_match")]


def test_between_two_keys_of_a_long_clip_the_anchored_chains_keep_up():
    """The (49, 40, 72) clip with keys on 8 and 40 at 3 levels: the device gives the restatement's bits, whose lowest per-frame IoU
    with the true disc is 0.871, and propagate_keys on the same input the plain restatement's, 0.737 (frame 23)."""
    images, truth, plain_want, want = gap_drift_case()
    t, m = _dev(images), _dev(truth[[8, 40]].astype(np.float32))
    got = propagate_keys_anchored.propagate_keys_anchored(t, m, [8, 40], 3, 2, 8, 2).cpu().numpy()
    plain = propagate_keys.propagate_keys(t, m, [8, 40], 3, 2, 8).cpu().numpy()
    _same_bits(got, want, "the anchored chains")
    _same_bits(plain, plain_want, "the plain chains")
    assert_the_two_iou_lines(truth, plain, got)


# ---- poison, a side stream, no read -----------------------------------------------------------------------------------------------------------
SCRATCH_PLANE, SCRATCH_KEYS = (40, 70), [1, 4]                          # an edge chain either side, a gap of two frames


@pytest.mark.parametrize("poison", [0x00, 0xFF], ids=lambda b: f"0x{b:02X}")
def test_the_call_under_poison_equals_the_restatement(poison, monkeypatch):
    want = _want(SCRATCH_PLANE, SCRATCH_KEYS)
    filled = poisoned_empty(monkeypatch, poison)
    got = _run(SCRATCH_PLANE, SCRATCH_KEYS)
    assert filled                                                      # the call's buffers did come through the poison
    _same_bits(got.cpu().numpy(), want, ("poison", poison))


def test_the_call_on_a_held_back_side_stream_reads_nothing_back(monkeypatch):
    """tests/test_gpu_motion_scratch.py's test of the same name, for this call: made on a side stream behind a delay whose event
    is not done when the call returns, so the call neither read from the device nor synchronised; every launch waited on that
    stream behind the poison fills of its buffers, or the bits differ; and nothing is left on the null stream."""
    want = _want(SCRATCH_PLANE, SCRATCH_KEYS)
    images, _, _, painted = _clip(SCRATCH_PLANE)
    t, m = _dev(images), _dev(painted[SCRATCH_KEYS])                   # built on the default stream
    run = lambda: propagate_keys_anchored.propagate_keys_anchored(t, m, SCRATCH_KEYS, LEVELS, SEARCH, SMOOTH, ANCHOR)    # noqa: E731
    cycles = int(_spin_cycles_per_ms() * DELAY_MS)
    torch.cuda.synchronize()
    filled = poisoned_empty(monkeypatch, 0xFF)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        run()                                                          # loads the kernels and fills this stream's pool
        side.synchronize()
        del filled[:]
        done = torch.cuda.Event()
        torch.cuda._sleep(cycles)
        done.record(side)
        start = time.perf_counter()
        got = run()
        held = not done.query()                                        # directly behind the call, before anything synchronises
        idle = torch.cuda.default_stream().query()
        call_ms = (time.perf_counter() - start) * 1e3
    print(f"propagate_keys_anchored: call behind the delay {call_ms:.2f} ms of host time; delay {DELAY_MS} ms")
    assert held, f"the call returned after {call_ms:.2f} ms with the {DELAY_MS} ms delay in front of it done"
    assert idle, "the call left work on the null stream"
    assert filled
    side.synchronize()
    _same_bits(got.cpu().numpy(), want, "side stream")


def test_node_returns_what_the_module_returns():
    plane, keys = (40, 70), [0, 3, 6]
    images, _, _, painted = _clip(plane)
    masks = painted[keys]
    node = propagate_keys_anchored_nodes.LanPaint_VideoMaskPropagateKeysAnchored()
    want = _run(plane, keys)
    out, = node.propagate(torch.from_numpy(images), torch.from_numpy(masks), "0, 3 6", LEVELS, SEARCH, SMOOTH, ANCHOR)
    assert not out.is_cuda and out.dtype == torch.float32
    _equal(out, want.cpu(), "host in, host out")
    out, = node.propagate(_dev(images), _dev(masks), "0,3,6", LEVELS, SEARCH, SMOOTH, ANCHOR)
    assert out.is_cuda
    _equal(out, want, "device in, device out")
    out, = node.propagate(torch.from_numpy(images), torch.from_numpy(masks[:1]))      # the defaults: key 0, levels 4, 2, 8, anchor 2
    _equal(out, propagate_anchored.propagate_masks_anchored(_dev(images), _dev(masks[0])).cpu(), "defaults")
    out, = node.propagate(_dev(images), _dev(masks), "0,3,6", LEVELS, SEARCH, SMOOTH, 0)
    _equal(out, propagate_keys.propagate_keys(_dev(images), _dev(masks), keys, LEVELS, SEARCH, SMOOTH), "anchor 0")
    assert propagate.MAX_SEARCH == propagate_keys_anchored.MAX_ANCHOR
