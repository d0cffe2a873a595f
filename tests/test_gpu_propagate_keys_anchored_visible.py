"""The anchored occlusion-aware video mask propagate from several keyframes on the MI355X
(lanpaint_amd.propagate_keys_anchored_visible; the gated form of lp_prop_match_batch, lp_prop_anchor_match_kernel<true> in
csrc/propagate_kernel.hip) against the numpy restatements tests/propagate_keys_anchored_visible_ref.py and
tests/propagate_anchored_visible_ref.py and against the single entry.  The rule is integer arithmetic, so every comparison covers
every element and has no tolerance.  Without the feature this file fails at its imports."""
import functools
import time

import numpy as np
import pytest
import torch

from lanpaint_amd import (_cabi, propagate_anchored_visible, propagate_keys, propagate_keys_anchored, propagate_keys_anchored_visible,
                          propagate_keys_anchored_visible_nodes, propagate_keys_visible)
from tests import propagate_anchored_visible_ref as avref
from tests import propagate_keys_anchored_visible_ref as kavref
from tests import propagate_ref as ref
from tests.compare import _same_bits, _same_ints as _same
from tests.device import DELAY_MS, DEV, _dev, _equal, _spin_cycles_per_ms
from tests.helpers import record_launches
from tests.inputs import (BATCH_PLANES, JOB_MASKS, KEYS_ANCHORED_CLIPS as CLIPS, MASKS, _job, _job_field, _keys_anchored_clip as _clip,
                          _soft, _video)
from tests.motion_checks import _offset_view
from tests.poison import poisoned_empty
from tests.propagate_scenes import assert_the_keys_quality_lines as assert_the_quality_lines, keys_quality_case as quality_case

pytestmark = pytest.mark.gpu
LEVELS, SEARCH, SMOOTH, ANCHOR, OCCLUSION = 3, 2, 8, 2, 16
STEP = ["lp_prop_match_batch", "lp_prop_fill_batch"] * LEVELS + ["lp_prop_advance_batch", "lp_prop_match_batch", "lp_prop_fill_batch",
                                                                  "lp_prop_advance_batch", "lp_prop_visible_batch", "lp_prop_occlude_batch"]
SINGLE = ("lp_prop_match", "lp_prop_fill", "lp_prop_advance", "lp_prop_visible", "lp_prop_occlude", "lp_prop_anchor_match",
          "lp_prop_anchor_match_gated")

# ---- the batched gated match ------------------------------------------------------------------------------------------------------------
NUMBERS = [(1, 0, 1), (2, 8, 16), (7, 64, 255)]                        # anchor, smooth, occlusion


@functools.lru_cache(maxsize=None)
def _gated_field(H, W, i, anchor, smooth, occlusion):
    P, Yt, Yk, m = _job(H, W, i)
    return avref.gated_anchor_field(P.astype(np.int64), Yt, Yk, m, anchor, smooth, occlusion)


def _rows(H, W, jobs, levels):
    """The jobs of a launch on the device, odd ones 4 bytes into their buffers: (key, tgt, mpyr, pos) per job, and the planes the
    single entry takes."""
    stride = _cabi.prop_pyramid_ws_bytes(1, H, W, levels)
    rows, planes = [], []
    for i in range(jobs):
        P, Yt, Yk, m = _job(H, W, i)
        off = 4 * (i & 1)
        key, tgt, mpyr, pos = _offset_view(Yk, off, stride), _offset_view(Yt, off, stride), _offset_view(m, off, stride), _offset_view(P, off)
        assert all(t.data_ptr() % 16 == off for t in (key, tgt, mpyr, pos))
        rows.append((key, tgt, mpyr, pos))
        planes.append([t[:H * W].view(H, W) for t in (tgt, key, mpyr)])
    return rows, planes


@pytest.mark.parametrize("plane", BATCH_PLANES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("jobs", [1, 2, 5, 32])
def test_the_batched_gated_match_equals_the_single_entry_and_the_restatement(plane, jobs, monkeypatch):
    """Odd jobs lie 4 bytes into their buffers: on (40, 72) they take the scalar path and the even ones the vector path, in one
    launch.  The outputs come poisoned, so a cell that nobody writes shows.  Every job of every launch against
    lp_prop_anchor_match_gated and against the restatement, at all three sets of numbers; a job's restatement is made once and
    shared by the launches that hold the job."""
    H, W = plane
    gh, gw = _cabi.prop_grid(H, W)
    for levels, (anchor, smooth, occlusion) in zip((1, 3, 2), NUMBERS):
        rows, planes = _rows(H, W, jobs, levels)
        filled = poisoned_empty(monkeypatch, 0xFF)
        got = propagate_keys.anchor_field_batch(rows, H, W, levels, anchor, smooth, occlusion)
        assert len(got) == jobs and len(filled) == 2 * jobs           # no third plane is allocated
        monkeypatch.undo()
        for i in range(jobs):
            what = (plane, jobs, "levels", levels, "anchor", anchor, "smooth", smooth, "occlusion", occlusion, "job", i)
            vec, valid = got[i]
            assert vec.dtype == valid.dtype == torch.int32 and tuple(vec.shape) == (gh, gw, 2) and tuple(valid.shape) == (gh, gw)
            tgt, key, bits = planes[i]
            want_vec, want_valid, want_gated = propagate_anchored_visible.gated_anchor_field(rows[i][3], tgt, key, bits, anchor, smooth,
                                                                                             occlusion)
            _equal(vec, want_vec, (*what, "vec against lp_prop_anchor_match_gated"))
            _equal(valid, want_valid, (*what, "valid against lp_prop_anchor_match_gated"))
            assert not (want_valid & want_gated).any() and not vec[want_gated != 0].any(), what
            ref_vec, ref_valid, ref_gated = _gated_field(H, W, i, anchor, smooth, occlusion)
            _same(valid.cpu().numpy(), ref_valid, (*what, "valid"))
            _same(vec.cpu().numpy(), ref_vec, (*what, "vec"))
            _same(want_gated.cpu().numpy(), ref_gated, (*what, "the single entry's gated"))
            if JOB_MASKS[i % len(JOB_MASKS)] in ("15 pixels", "empty"):   # no live block: all zero
                assert not vec.any() and not valid.any(), what


def test_the_gated_jobs_take_both_branches_and_the_ungated_form_keeps_its_bits(monkeypatch):
    """What the comparison above rests on, on the restatement: at (2, 8, 16) job 3 has gated and valid blocks side by side, at
    occlusion 1 every live block is gated, at 255 none; the fields are not all zero.  And in this process, behind gated launches,
    reserved0 = LP_PROP_MATCH_WARPED_KEY still gives the ungated bits; the library's refusals on real buffers."""
    for plane, gated_blocks, valid_blocks in (((33, 70), 12, 33), ((40, 72), 5, 40)):
        vec, valid, gated = _gated_field(*plane, 3, 2, 8, 16)
        assert (int(gated.sum()), int(valid.sum())) == (gated_blocks, valid_blocks) and vec.any(), plane
        assert not vec[gated != 0].any() and vec[valid].any(), plane
        for anchor, smooth, occlusion in NUMBERS[1:]:                   # valid and invalid blocks side by side among the first jobs
            fields = [_gated_field(*plane, i, anchor, smooth, occlusion) for i in range(5)]
            assert any(ok.any() and not ok.all() for _, ok, _ in fields), (plane, anchor)
        assert any((_gated_field(*plane, i, 7, 64, 255)[0] % 16 != 0).any() for i in range(5)), plane      # the sub-pixel step
        # beyond the first jobs: 5, 8 and 11 have "outside" positions under masks with live blocks, 6 and 18 gated and valid blocks
        for i in (5, 8, 11):
            _, valid, gated = _gated_field(*plane, i, 2, 8, 16)
            assert (valid | (gated != 0)).any(), (plane, i)
        for i in (6, 18):
            _, valid, gated = _gated_field(*plane, i, 2, 8, 16)
            assert gated.any() and valid.any(), (plane, i)
        _, valid, gated = _gated_field(*plane, 3, 1, 0, 1)
        assert int(gated.sum()) == 45 and not valid.any(), plane        # every live block
        _, valid, gated = _gated_field(*plane, 3, 7, 64, 255)
        assert not gated.any() and int(valid.sum()) == 45, plane
    for H, W in ((33, 70), (40, 72)):                                  # the scalar path, and both paths in one launch
        for levels, (anchor, smooth, occlusion) in zip((1, 3, 2), NUMBERS):
            rows, _ = _rows(H, W, 5, levels)
            propagate_keys.anchor_field_batch(rows, H, W, levels, anchor, smooth, occlusion)
            filled = poisoned_empty(monkeypatch, 0xFF)
            plain = propagate_keys.anchor_field_batch(rows, H, W, levels, anchor, smooth)
            monkeypatch.undo()
            assert filled
            for i, (vec, valid) in enumerate(plain):
                ref_vec, ref_valid = _job_field(H, W, i, anchor, smooth)
                _same(valid.cpu().numpy(), ref_valid, ("ungated valid", (H, W), anchor, i))
                _same(vec.cpu().numpy(), ref_vec, ("ungated vec", (H, W), anchor, i))
    H, W = 40, 72
    stride = _cabi.prop_pyramid_ws_bytes(1, H, W, 2)
    row = torch.zeros(stride, dtype=torch.uint8, device=DEV)
    pos = torch.zeros((H, W, 2), dtype=torch.int32, device=DEV)
    assert len(propagate_keys.anchor_field_batch([(row, row, row, pos)] * 32, H, W, 2, 1, 0, 255)) == 32
    for bad in (dict(occlusion=-1), dict(occlusion=256), dict(anchor=0), dict(anchor=8)):
        with pytest.raises(ValueError):
            propagate_keys.anchor_field_batch([(row, row, row, pos)], H, W, **{"levels": 2, "anchor": 2, "smooth": 8, "occlusion": 16, **bad})
    vec, valid = torch.zeros((5, 9, 2), dtype=torch.int32, device=DEV), torch.zeros((5, 9), dtype=torch.int32, device=DEV)
    lib = _cabi.load()
    for job in ((row, row, row, pos, pos, valid), (row, row, row, pos, vec, vec), (row, row, row, None, vec, valid)):
        table = propagate_keys.job_table([job], "refusals")
        d = _cabi.LpPropMatchBatchDesc(H, W, 2, 0, 2, 8, 1, _cabi.LP_PROP_MATCH_GATED(16), table.ctypes.data)
        assert lib.lp_prop_match_batch(d, None) == _cabi.LP_E_INVALID
    table = propagate_keys.job_table([(row, row, row, pos, vec, valid)], "refusals")
    for form in (_cabi.LP_PROP_MATCH_GATED(16) | 2, _cabi.LP_PROP_MATCH_GATED(16) | (1 << 16), 16 << 8):
        d = _cabi.LpPropMatchBatchDesc(H, W, 2, 0, 2, 8, 1, form, table.ctypes.data)
        assert lib.lp_prop_match_batch(d, None) == _cabi.LP_E_INVALID
    torch.cuda.synchronize()


# ---- the whole call ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _longest_chain(plane, half, k, d):
    """The longest anchored occlusion-aware chain from key k in direction d; a shorter chain is its beginning."""
    images, _, pyr, painted = _clip(plane, half)
    F = len(images)
    return kavref.run_chain(pyr, ref.binarise(painted[k]), k, d, k if d < 0 else F - 1 - k, LEVELS, SEARCH, SMOOTH, ANCHOR, OCCLUSION)


def _want(plane, keys, half=False):
    images, _, _, painted = _clip(plane, half)

    def chain(i, k, d, length):
        frames, counts = _longest_chain(plane, half, k, d)
        return {t: v for t, v in frames.items() if abs(t - k) <= length}, counts[:length + 1]
    return kavref.propagate_keys_anchored_visible_ref(images, painted[keys], keys, LEVELS, SEARCH, SMOOTH, ANCHOR, OCCLUSION, chain=chain)


def _call(t, m, keys, anchor=ANCHOR, occlusion=OCCLUSION):
    return propagate_keys_anchored_visible.propagate_keys_anchored_visible(t, m, keys, LEVELS, SEARCH, SMOOTH, anchor, occlusion)


def _run(plane, keys, half=False):
    images, _, _, painted = _clip(plane, half)
    t = _dev(images).half() if half else _dev(images)
    got = _call(t, _dev(painted[keys]), keys)
    for g in got:
        assert g.is_cuda and g.dtype == torch.float32 and tuple(g.shape) == (len(images), *plane)
    return got


def _same_pair(got, want, what):
    for g, w, name in zip(got, want, ("mask", "hidden")):
        _same_bits(g.cpu().numpy(), w, (*what, name))                  # 0 differing elements


def _equal_pair(got, want, what):
    for g, w, name in zip(got, want, ("mask", "hidden")):
        _equal(g, w, (*what, name))


@pytest.mark.parametrize("plane", list(CLIPS), ids=lambda s: "x".join(map(str, s)))
def test_the_whole_call_equals_the_restatement_for_every_key_set(plane):
    H, W = plane
    F, key_sets = CLIPS[plane]
    images, _, _, painted = _clip(plane)
    t = _dev(images)
    single = propagate_anchored_visible.propagate_masks_anchored_visible
    for keys in key_sets:
        got, want = _run(plane, keys), _want(plane, keys)
        _same_pair(got, want, (plane, keys))
        for k in keys:                                                 # a key frame: its painting and a zero hidden
            _same_bits(want[0][k], ref.binarise(painted[k]).astype(np.float32), "a key frame is its binarised mask")
            assert not want[1][k].any()
        total = (got[0].double() + got[1].double()) * 256
        assert torch.equal(total, total.round()) and float(total.min()) >= 0 and float(total.max()) <= 256
        masks = [_dev(painted[k]) for k in keys]
        first = single(t, masks[0], keys[0], LEVELS, SEARCH, SMOOTH, ANCHOR, OCCLUSION)
        if len(keys) == 1:                                             # K = 1 is the single-key form, and [H, W] is accepted
            _equal_pair(got, first, ("K = 1", plane, keys))
            _equal_pair(_call(t, masks[0], keys), first, ("[H, W]",))
        else:                                                          # outside the keys: the single-key chain of the nearest key
            last = single(t, masks[-1], keys[-1], LEVELS, SEARCH, SMOOTH, ANCHOR, OCCLUSION)
            _equal_pair([g[:keys[0] + 1] for g in got], [f[:keys[0] + 1] for f in first], ("in front of the first key", plane, keys))
            _equal_pair([g[keys[-1]:] for g in got], [f[keys[-1]:] for f in last], ("behind the last key", plane, keys))
            per_frame = np.full((F, H, W), 0.75, np.float32)           # what is not on a key frame is not read
            per_frame[keys] = painted[keys]
            _equal_pair(_call(t, _dev(per_frame), keys), got, ("[F, H, W]",))
    for plane_keys in (((9, 7), [0, 2, 5]), ((40, 70), [0, 6])):       # fp16 images: the restatement on the half-rounded values
        if plane_keys[0] == plane:
            _same_pair(_run(plane, plane_keys[1], half=True), _want(plane, plane_keys[1], half=True), ("fp16", *plane_keys))
    if plane == (40, 70):                                              # both refinements are at work: neither existing form's bits
        m = _dev(painted[[0, 6]])
        got = _run(plane, [0, 6])
        assert not torch.equal(got[0], propagate_keys_visible.propagate_keys_visible(t, m, [0, 6], LEVELS, SEARCH, SMOOTH, OCCLUSION)[0])
        assert not torch.equal(got[0], propagate_keys_anchored.propagate_keys_anchored(t, m, [0, 6], LEVELS, SEARCH, SMOOTH, ANCHOR))


def test_the_off_routes_make_no_new_launch(monkeypatch):
    plane, keys = (40, 70), [0, 3, 6]
    images, _, _, painted = _clip(plane)
    t, m = _dev(images), _dev(painted[keys])
    names = record_launches(monkeypatch, propagate_keys_anchored_visible, propagate_keys_visible, propagate_keys_anchored, propagate_keys)
    routes = ((0, OCCLUSION, lambda: propagate_keys_visible.propagate_keys_visible(t, m, keys, LEVELS, SEARCH, SMOOTH, OCCLUSION)),
              (ANCHOR, 0, lambda: propagate_keys_anchored.propagate_keys_anchored(t, m, keys, LEVELS, SEARCH, SMOOTH, ANCHOR)),
              (0, 0, lambda: propagate_keys.propagate_keys(t, m, keys, LEVELS, SEARCH, SMOOTH)))
    for anchor, occlusion, other in routes:
        del names[:]
        want = other()
        theirs = list(names)
        del names[:]
        got = _call(t, m, keys, anchor, occlusion)
        assert names == theirs, (anchor, occlusion)                    # nothing but what the other form launches itself
        if torch.is_tensor(want):
            assert torch.equal(got[0], want) and not got[1].any(), (anchor, occlusion)
        else:
            _equal_pair(got, want, ("off", anchor, occlusion))
    del names[:]
    _call(t, m, keys)
    assert [n for n in names if n.endswith("_batch")][1:] == STEP * 2 and names.count("lp_prop_occlude_batch") == 3   # + the keys' counts
    assert not [n for n in names if n in SINGLE]
    assert names.count("lp_prop_merge_visible") == 2 and names.count("lp_prop_luma") == 1


def test_a_still_video_and_empty_keys():
    H, W, F = 40, 70, 7
    still = _dev(np.repeat(_video(1, H, W), F, axis=0))
    soft = _soft(H, W, 3)
    for anchor, occlusion in ((2, 16), (7, 1)):
        got = _call(still, _dev(np.repeat(soft[None], 3, axis=0)), [0, 2, 6], anchor, occlusion)
        _same_bits(got[0].cpu().numpy(), np.repeat(ref.binarise(soft).astype(np.float32)[None], F, axis=0), ("a still video", anchor))
        assert not got[1].any()
    moving = _dev(_clip((40, 70))[0])
    for keys in ([0, 6], [1, 4], [0, 3, 6]):
        got = _call(moving, torch.zeros((len(keys), H, W), device=DEV), keys, 7, 1)
        assert not got[0].any() and not got[1].any(), keys             # exactly 0.0 and 0.0


def test_more_chains_than_one_launch_holds(monkeypatch):
    """A key on every even frame of 36: 35 chains of one step, so every stage of the step takes two launches (32 + 3)."""
    F, H, W = 36, 24, 40
    keys = list(range(0, F, 2))
    assert len(propagate_keys.chain_plan(F, keys)) == 35
    images = _video(F, H, W, 3, seed=2)
    masks = np.stack([MASKS[("disc", "soft", "full")[k % 3]](H, W, k) for k in keys])
    names = record_launches(monkeypatch, propagate_keys_anchored_visible, propagate_keys_visible, propagate_keys)
    got = _call(_dev(images), _dev(masks), keys)
    batched = [n for n in names if n.endswith("_batch")]
    assert batched == ["lp_prop_occlude_batch"] * 2 + STEP * 2 and names.count("lp_prop_merge_visible") == 17    # 34 counted keys
    _same_pair(got, kavref.propagate_keys_anchored_visible_ref(images, masks, keys, LEVELS, SEARCH, SMOOTH, ANCHOR, OCCLUSION), ("35 chains",))


def test_what_the_call_keeps_must_fit_the_cap_raw_pos_included(monkeypatch):
    """F = 7 at 40 x 70 with keys on both ends: propagate_keys_visible's sum for 5 in-between frames and 2 chains, plus a position
    map (two planes) per chain.  One byte short raises and names both numbers; exactly enough gives the same bits."""
    plane, keys = (40, 70), [0, 6]
    images, _, _, painted = _clip(plane)
    t, m = _dev(images), _dev(painted[keys])
    want = _call(t, m, keys)
    assert _cabi.prop_grid(*plane) == (5, 9)
    pixels, cells = 40 * 70 * 4, 5 * 9 * 4
    kept = 5 * 2 * (pixels + cells) + 3 * (pixels + cells) + 2 * 2 * pixels
    monkeypatch.setattr(propagate_keys_anchored_visible, "WS_CAP_BYTES", kept - 1)
    with pytest.raises(ValueError, match=f"the position maps of 2 anchored chains take {kept} bytes.*{kept - 1}"):
        _call(t, m, keys)
    propagate_keys_visible.propagate_keys_visible(t, m, keys, LEVELS, SEARCH, SMOOTH, OCCLUSION)       # its own cap is its own
    monkeypatch.setattr(propagate_keys_anchored_visible, "WS_CAP_BYTES", kept)
    _equal_pair(_call(t, m, keys), want, ("exactly enough",))


@pytest.mark.parametrize("name", ["A", "B", "disc"])
def test_the_quality_clips_on_the_device(name):
    """The bits are the restatement's; then tests/test_propagate_keys_anchored_visible_host.py's lines on the device's outputs."""
    images, masks, keys, levels, truth, want, _, _, _ = quality_case(name)
    t, m = _dev(images), _dev(masks)
    got = propagate_keys_anchored_visible.propagate_keys_anchored_visible(t, m, keys, levels, 2, 8, 2, 16)
    _same_pair(got, want, (name,))
    keys_visible = propagate_keys_visible.propagate_keys_visible(t, m, keys, levels, 2, 8, 16)
    keys_anchored = propagate_keys_anchored.propagate_keys_anchored(t, m, keys, levels, 2, 8, 2)
    assert_the_quality_lines(name, truth, [g.cpu().numpy() for g in got], [g.cpu().numpy() for g in keys_visible],
                             keys_anchored.cpu().numpy())


# ---- poison, a side stream, no read, the node ------------------------------------------------------------------------------------------------
SCRATCH_PLANE, SCRATCH_KEYS = (40, 70), [1, 4]                          # an edge chain either side, a gap of two frames


@pytest.mark.parametrize("poison", [0x00, 0xFF], ids=lambda b: f"0x{b:02X}")
def test_the_call_under_poison_equals_the_restatement(poison, monkeypatch):
    want = _want(SCRATCH_PLANE, SCRATCH_KEYS)
    filled = poisoned_empty(monkeypatch, poison)
    got = _run(SCRATCH_PLANE, SCRATCH_KEYS)
    assert filled                                                      # the call's buffers did come through the poison
    _same_pair(got, want, ("poison", poison))


def test_the_call_on_a_held_back_side_stream_reads_nothing_back(monkeypatch):
    """tests/test_gpu_motion_scratch.py's test of the same name, for this call: made on a side stream behind a delay whose event
    is not done when the call returns, so the call neither read from the device nor synchronised; every launch waited on that
    stream behind the poison fills of its buffers, or the bits differ; and nothing is left on the null stream."""
    want = _want(SCRATCH_PLANE, SCRATCH_KEYS)
    images, _, _, painted = _clip(SCRATCH_PLANE)
    t, m = _dev(images), _dev(painted[SCRATCH_KEYS])                   # built on the default stream
    run = lambda: _call(t, m, SCRATCH_KEYS)                            # noqa: E731
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
    print(f"propagate_keys_anchored_visible: call behind the delay {call_ms:.2f} ms of host time; delay {DELAY_MS} ms")
    assert held, f"the call returned after {call_ms:.2f} ms with the {DELAY_MS} ms delay in front of it done"
    assert idle, "the call left work on the null stream"
    assert filled
    side.synchronize()
    _same_pair(got, want, ("side stream",))


def test_node_returns_what_the_module_returns():
    plane, keys = (40, 70), [0, 3, 6]
    images, _, _, painted = _clip(plane)
    masks = painted[keys]
    node = propagate_keys_anchored_visible_nodes.LanPaint_VideoMaskPropagateKeysAnchoredVisible()
    per_shot = propagate_keys_anchored_visible_nodes.LanPaint_VideoMaskPropagateKeysAnchoredVisibleShots()
    want = _run(plane, keys)
    out = node.propagate(torch.from_numpy(images), torch.from_numpy(masks), "0, 3 6", LEVELS, SEARCH, SMOOTH, ANCHOR, OCCLUSION)
    assert len(out) == 2 and not out[0].is_cuda and not out[1].is_cuda and out[0].dtype == out[1].dtype == torch.float32
    _equal_pair(out, [w.cpu() for w in want], ("host in, host out",))
    out = node.propagate(_dev(images), _dev(masks), "0,3,6", LEVELS, SEARCH, SMOOTH, ANCHOR, OCCLUSION)
    assert out[0].is_cuda and out[1].is_cuda
    _equal_pair(out, want, ("device in, device out",))
    out = node.propagate(torch.from_numpy(images), torch.from_numpy(masks[:1]))       # the defaults: key 0, levels 4, 2, 8, 2, 16
    _equal_pair(out, [w.cpu() for w in propagate_anchored_visible.propagate_masks_anchored_visible(_dev(images), _dev(masks[0]))], ("defaults",))
    _equal_pair(per_shot.propagate(_dev(images), _dev(masks), "0,3,6", LEVELS, SEARCH, SMOOTH, ANCHOR, OCCLUSION), want, ("no shots",))
    # two shots, frames 0..3 with keys 0 and 3 and frames 4..6 with key 6: each the call on its own frames and keys
    out = per_shot.propagate(_dev(images), _dev(masks), "0,3,6", LEVELS, SEARCH, SMOOTH, ANCHOR, OCCLUSION, shots=[(0, 4), (4, 7)])
    t = _dev(images)
    head, tail = _call(t[:4], _dev(masks[:2]), [0, 3]), _call(t[4:], _dev(masks[2:]), [2])
    _equal_pair(out, [torch.cat([h, w]) for h, w in zip(head, tail)], ("two shots",))
