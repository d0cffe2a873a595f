"""The motion family on the MI355X where its other suites do not look: scratch and outputs that hold a poison before the call, a
side stream that is held back while the call is made, and the docstrings' "no device -> host read".

The ten public calls (propagate_masks, propagate_masks_visible, propagate_masks_anchored, propagate_keys, propagate_keys_visible,
temporal_fill, temporal_fill_checked, temporal_smooth, temporal_smooth_robust, detect_shots) and the stage functions that allocate
their own results run with every `torch.empty` / `torch.empty_like` filled with 0x00 and with 0xFF (tests/poison.py).  Every buffer
of the family comes from there, outputs included, so a cell that is read before it is written, an element nobody writes or pyramid
padding that reaches a result shows as different bits.  Each comparison is the one the call's own suite applies to the whole call
against its numpy restatement -- bit for bit, NaN matching NaN in the fills and the smooths -- and no tolerance is added.

0x00 and 0xFF (-1) and nothing wilder: the kernels clamp or range-check every index they derive from a buffer's value (a parent
vector, a position map, a carried origin's frame, a field), and both values stay next to the buffer should one ever be used raw.
"""
import functools
import json
import os
import time

import numpy as np
import pytest
import torch

from lanpaint_amd import (_cabi, propagate, propagate_anchored, propagate_anchored_visible, propagate_keys, propagate_keys_visible,
                          propagate_visible, shots, temporal_fill, temporal_fill_checked, temporal_smooth, temporal_smooth_robust)
from tests import inputs, motion_checks
from tests import propagate_anchored_ref as aref
from tests import propagate_keys_ref as kref
from tests import propagate_keys_visible_ref as kvref
from tests import propagate_ref as ref
from tests import propagate_visible_ref as vref
from tests import shots_ref as shref
from tests import temporal_fill_checked_ref as cref
from tests import temporal_fill_ref as tref
from tests import temporal_smooth_ref as sref
from tests import temporal_smooth_robust_ref as rref
from tests.compare import _same_bits, _same_ints as _same
from tests.device import DELAY_MS, _dev, _levels_of, _spin_cycles_per_ms
from tests.helpers import GOLDEN_DIR, record_launches
from tests.inputs import LARGE, SMALL, _disc, _random_masks, _rng, _video
from tests.poison import POISONS, poison_id, poisoned_empty

pytestmark = pytest.mark.gpu

# F = 7 with the single key in the middle: three steps either way, so both buffers of every ping-pong pair are written and read.
# Keys on 1 and 4: an edge chain in front of the first key, a gap of two in-between frames with a forward and a backward chain, an
# edge chain behind the last key.
F, KEY, KEYS, SEARCH, SMOOTH, RADIUS, TOLERANCE = 7, 3, (1, 4), 2, 8, 2, 24
# the checked fill's default `agree` of 8 disputes nothing on these clips (counted on the restatement); 4 disputes 97 pixels on
# (23, 33) and 372 on (40, 70) and leaves all of 0, 1 and 2 in `witnesses`
AGREE = 4
# shot decision: every pair whose residual is a maximum among its two neighbours is a cut, so that `shot` is not all zero
DECISION = dict(threshold=1, hist=0, ratio=100, window=1)
CASES = [(SMALL, 3, "whole"), (SMALL, 3, "chunked"), (LARGE, 3, "whole"), (LARGE, 3, "chunked"), (SMALL, 1, "whole"), (SMALL, 6, "whole")]
case_id = lambda c: c if isinstance(c, str) else "x".join(map(str, c)) if isinstance(c, tuple) else f"levels{c}"    # noqa: E731


# ---- inputs and restatements, once per plane and mode ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(plane, mode):
    """(images [F, H, W, 3], the key mask, the two keys' masks, a mask per frame) in numpy, shared: not to be written to.  The
    keys' discs are moved so that on both planes, at 3 and 6 levels, exactly one chain of the gap is lost on some frame."""
    H, W = plane
    images = _video(F, H, W)
    if mode == "chunked":
        images = images.astype(np.float16).astype(np.float32)
    disc = _disc(H, W)
    keys = np.stack([np.roll(disc, (5 * k, -10 * k), (0, 1)) for k in KEYS])
    masks = _random_masks(F, H, W)
    for a in (images, disc, keys, masks):
        a.setflags(write=False)
    return images, disc, keys, masks


def _device_inputs(plane, mode):
    images, disc, keys, masks = (_dev(a) for a in _inputs(plane, mode))
    return (images.half() if mode == "chunked" else images), disc, keys, masks


@functools.lru_cache(maxsize=None)
def _want(call, plane, levels, mode):
    """The restatement's outputs of `call`, a tuple in the call's order."""
    images, disc, keys, masks = _inputs(plane, mode)
    if call == "propagate_masks":
        return (ref.propagate_ref(images, disc, KEY, levels, SEARCH, SMOOTH),)
    if call == "propagate_masks_visible":
        return vref.propagate_visible_ref(images, disc, KEY, levels, SEARCH, SMOOTH, propagate_visible.DEFAULT_OCCLUSION)
    if call == "propagate_masks_anchored":
        return (aref.propagate_anchored_ref(images, disc, KEY, levels, SEARCH, SMOOTH, propagate_anchored.DEFAULT_ANCHOR),)
    if call == "propagate_keys":
        return (kref.propagate_keys_ref(images, keys, list(KEYS), levels, SEARCH, SMOOTH),)
    if call == "propagate_keys_visible":
        trace = {}
        want = kvref.propagate_keys_visible_ref(images, keys, list(KEYS), levels, SEARCH, SMOOTH, propagate_visible.DEFAULT_OCCLUSION, trace)
        if levels > 1:            # the keys' own counts decide nothing unless a chain is lost: one is, and on some frame alone
            assert any(a != b for a, b in trace["lost"].values()), trace["lost"]
        return want
    if call == "temporal_fill":
        return tref.temporal_fill_ref(images, masks, levels, SEARCH, SMOOTH, 0)
    if call == "temporal_fill_checked":
        want = cref.temporal_fill_checked_ref(images, masks, levels, SEARCH, SMOOTH, 0, AGREE)
        assert (want[2] == cref.DISPUTED).any() and {0, 1} <= set(np.unique(want[3]))
        assert levels == 1 or (want[3] == 2).any()                    # with one level every tested block is disputed here
        return want
    if call == "temporal_smooth":
        return sref.temporal_smooth_ref(images, masks, RADIUS, TOLERANCE, "background", levels, SEARCH, SMOOTH)
    if call == "temporal_smooth_robust":
        want = rref.temporal_smooth_robust_ref(images, masks, RADIUS, TOLERANCE, "background", levels, SEARCH, SMOOTH)
        assert (want[2] == 1).any()
        return want
    assert call == "detect_shots"
    shot, score = shref.detect_shots(images, DECISION["threshold"], DECISION["hist"], DECISION["ratio"], DECISION["window"], levels - 1, SEARCH)
    assert shot[-1] > 0
    return shot, score


def _run(call, levels, images, disc, keys, masks):
    """The device's outputs of `call`, a tuple in the call's order."""
    if call == "propagate_masks":
        return (propagate.propagate_masks(images, disc, KEY, levels, SEARCH, SMOOTH),)
    if call == "propagate_masks_visible":
        return propagate_visible.propagate_masks_visible(images, disc, KEY, levels, SEARCH, SMOOTH)              # the default occlusion
    if call == "propagate_masks_anchored":
        return (propagate_anchored.propagate_masks_anchored(images, disc, KEY, levels, SEARCH, SMOOTH),)
    if call == "propagate_keys":
        return (propagate_keys.propagate_keys(images, keys, list(KEYS), levels, SEARCH, SMOOTH),)
    if call == "propagate_keys_visible":
        return propagate_keys_visible.propagate_keys_visible(images, keys, list(KEYS), levels, SEARCH, SMOOTH)   # the default, not 0
    if call == "temporal_fill":
        return temporal_fill.temporal_fill(images, masks, levels, SEARCH, SMOOTH)
    if call == "temporal_fill_checked":
        return temporal_fill_checked.temporal_fill_checked(images, masks, levels, SEARCH, SMOOTH, 0, AGREE)
    if call == "temporal_smooth":
        return temporal_smooth.temporal_smooth(images, masks, RADIUS, TOLERANCE, "background", levels, SEARCH, SMOOTH)
    if call == "temporal_smooth_robust":
        return temporal_smooth_robust.temporal_smooth_robust(images, masks, RADIUS, TOLERANCE, "background", levels, SEARCH, SMOOTH)
    assert call == "detect_shots"
    return shots.detect_shots(images, level=levels - 1, search=SEARCH, **DECISION)


def _compare(call, got, want, what):
    """The comparison the call's own suite applies to the whole call."""
    assert len(got) == len(want), what
    if call.startswith("propagate"):
        for g, w, name in zip(got, want, ("mask", "hidden")):
            assert g.is_cuda and g.dtype == torch.float32
            _same_bits(g.cpu().numpy(), w, (what, name))
    elif call == "detect_shots":
        shot, score = got
        assert shot.is_cuda and shot.dtype == torch.int32 and score.is_cuda and score.dtype == torch.int64
        _same(score.cpu().numpy(), want[1], (what, "score"))
        _same(shot.cpu().numpy(), want[0], (what, "shot"))
    else:
        {"temporal_fill": motion_checks._check_fill_whole, "temporal_fill_checked": motion_checks._check_checked_whole,
         "temporal_smooth": motion_checks._check_smooth, "temporal_smooth_robust": motion_checks._check_robust_smooth}[call](got, want, what)


MODULES = (propagate, propagate_visible, propagate_anchored, propagate_keys, propagate_keys_visible, temporal_fill,
           temporal_fill_checked, temporal_smooth, temporal_smooth_robust, shots)
CALLS = ["propagate_masks", "propagate_masks_visible", "propagate_masks_anchored", "propagate_keys", "propagate_keys_visible",
         "temporal_fill", "temporal_fill_checked", "temporal_smooth", "temporal_smooth_robust", "detect_shots"]


def _lower_caps(monkeypatch, H, W, levels):
    """tests/test_gpu_motion_launches.py's rule for this clip: a chunk holds one or two frames or steps.  What
    propagate_keys_visible keeps is again 9 planes and grids: 2 in-between frames of 2 chains, and 4 chains and one."""
    stride = _cabi.prop_pyramid_ws_bytes(1, H, W, levels)
    gh, gw = _cabi.prop_grid(H, W)
    plane, cells = H * W * 4, gh * gw * 4
    monkeypatch.setattr(propagate, "WS_CAP_BYTES", 2 * stride + 8)                    # a frame and its fp32 copy: one frame a chunk
    monkeypatch.setattr(propagate_keys, "WS_CAP_BYTES", F * stride + 8)               # the clip's pyramids; a frame a conversion
    monkeypatch.setattr(propagate_keys_visible, "WS_CAP_BYTES", 9 * (plane + cells))
    monkeypatch.setattr(temporal_fill, "WS_CAP_BYTES", 2 * stride + 2 * (2 * stride + gh * gw * 8) + 8)       # two steps a chunk
    monkeypatch.setattr(temporal_smooth, "WS_CAP_BYTES", (2 * RADIUS + 1) * (2 * stride + 2 * gh * gw * 8) + 8)   # one frame a chunk
    monkeypatch.setattr(shots, "WS_CAP_BYTES", 1)                                     # one pair a chunk


# ---- B: the ten calls under poison -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", POISONS, ids=poison_id)
@pytest.mark.parametrize("plane,levels,mode", CASES, ids=case_id)
@pytest.mark.parametrize("call", CALLS)
def test_the_call_under_poison_equals_the_restatement(call, plane, levels, mode, poison, monkeypatch):
    want = _want(call, plane, levels, mode)
    args = _device_inputs(plane, mode)
    if mode == "chunked":
        _lower_caps(monkeypatch, *plane, levels)
    names = record_launches(monkeypatch, *MODULES)
    filled = poisoned_empty(monkeypatch, poison)
    got = _run(call, levels, *args)
    assert filled                                                      # the call's buffers did come through the poison
    # whole: the clip's pyramids in one launch, or one per direction (the single-key forms); chunked: one per chunk or frame,
    # at the fewest the fills' five (three ranges of frames forwards, the last of them again and two more backwards)
    lumas = names.count("lp_prop_luma")
    assert lumas <= 2 if mode == "whole" else lumas >= 5, (mode, lumas)
    _compare(call, got, want, (call, plane, levels, mode, poison_id(poison)))


# ---- B: what each propagate form allocates -------------------------------------------------------------------------------------------------
# The four single-key forms run on one step class with the refinements as options; each has to get the buffers it had as a class of
# its own and no more: the plain form no code, raw_mpyr, raw_pos, flags or gate, the visible form no raw_pos.  Their lists are the
# record of the last commit that had the four classes, taken on the MI355X (CHANGES.md has the command).  The two several-keys
# forms run on one chain class with the occlusion-aware form as an option, and the plain one has to get no raw_mpyr and no stack
# but `back`: their lists are the record of the last commit that had `VisibleChains`, taken the same way.
SINGLE_KEY_CALLS = {
    "propagate_masks": lambda images, mask: propagate.propagate_masks(images, mask, KEY, 3, SEARCH, SMOOTH),
    "propagate_masks_visible": lambda images, mask: propagate_visible.propagate_masks_visible(images, mask, KEY, 3, SEARCH, SMOOTH),
    "propagate_masks_anchored": lambda images, mask: propagate_anchored.propagate_masks_anchored(images, mask, KEY, 3, SEARCH, SMOOTH),
    "propagate_masks_anchored_visible":
        lambda images, mask: propagate_anchored_visible.propagate_masks_anchored_visible(images, mask, KEY, 3, SEARCH, SMOOTH),
}
KEYS_CALLS = {
    "propagate_keys": lambda images, keys: propagate_keys.propagate_keys(images, keys, list(KEYS), 3, SEARCH, SMOOTH),
    "propagate_keys_visible": lambda images, keys: propagate_keys_visible.propagate_keys_visible(images, keys, list(KEYS), 3, SEARCH, SMOOTH),
}
SCRATCH_FIXTURE = os.path.join(GOLDEN_DIR, "propagate_scratch_bytes.json")


def scratch_bytes(call, monkeypatch):
    """The sorted byte counts of every buffer the form `call` takes through `torch.empty` / `torch.empty_like` on the 7-frame fp32
    clip of (23, 33), key frame 3 or keys (1, 4), 3 levels, the caps as they are."""
    images, disc, keys, _ = _device_inputs(SMALL, "whole")
    filled = poisoned_empty(monkeypatch, 0xFF)
    if call in KEYS_CALLS:
        KEYS_CALLS[call](images, keys)
    else:
        SINGLE_KEY_CALLS[call](images, disc)
    torch.cuda.synchronize()
    return sorted(filled)


def record_scratch_bytes():
    """What SCRATCH_FIXTURE holds, from whichever lanpaint_amd is first on the path."""
    record = {}
    for call in (*SINGLE_KEY_CALLS, *KEYS_CALLS):
        with pytest.MonkeyPatch.context() as patch:
            record[call] = scratch_bytes(call, patch)
    return record


def _allocates_what_was_recorded(call, monkeypatch):
    with open(SCRATCH_FIXTURE) as f:
        want = json.load(f)[call]
    got = scratch_bytes(call, monkeypatch)
    print(f"{call}: {len(got)} buffers, {sum(got)} bytes; recorded {len(want)} buffers, {sum(want)} bytes")
    assert got == want, (call, got, want)


@pytest.mark.parametrize("call", list(SINGLE_KEY_CALLS))
def test_each_single_key_form_allocates_what_it_did_as_a_class_of_its_own(call, monkeypatch):
    _allocates_what_was_recorded(call, monkeypatch)


@pytest.mark.parametrize("call", list(KEYS_CALLS))
def test_each_several_keys_form_allocates_what_it_did_with_a_chain_class_of_its_own(call, monkeypatch):
    _allocates_what_was_recorded(call, monkeypatch)


# ---- B: the stage functions that allocate their own results, fed as their suites feed them, at (23, 33) -----------------------------------
H, W = SMALL
stage = pytest.mark.parametrize("poison", POISONS, ids=poison_id)


@stage
def test_key_mask_under_poison(poison, monkeypatch):
    filled = poisoned_empty(monkeypatch, poison)
    for form in ("disc", "soft", "wild"):
        mask = inputs.MASKS[form](H, W)
        bits = ref.binarise(mask)
        for levels in (1, 3, 6):
            mpyr, out = propagate.key_mask(_dev(mask), levels)
            _same_bits(out.cpu().numpy(), bits.astype(np.float32), ("key mask", form))
            for lv, (g, w) in enumerate(zip(_levels_of(mpyr, H, W, levels), ref.pyramid(bits, levels, ref.down_mask))):
                _same(g[0], w, ("mask pyramid", form, levels, lv))
    assert filled


@stage
def test_match_level_and_fill_median_under_poison(poison, monkeypatch):
    filled = poisoned_empty(monkeypatch, poison)
    for levels in (1, 3, 6):
        motion_checks._check_match(H, W, levels, SEARCH, SMOOTH, "random", "disc", (poison, levels))
    assert filled


@stage
def test_advance_under_poison(poison, monkeypatch):
    filled = poisoned_empty(monkeypatch, poison)
    vec, vec2, bits, P1, c1, P2, c2 = inputs._advance_case(H, W, 40)
    for levels in (1, 6):
        pos1, out1, mp1 = propagate.advance(_dev(vec), None, _dev(bits), levels)
        pos2, out2, mp2 = propagate.advance(_dev(vec2), pos1, _dev(bits), levels)
        for pos, out, mp, P, c in ((pos1, out1, mp1, P1, c1), (pos2, out2, mp2, P2, c2)):
            _same(pos.cpu().numpy(), P, ("positions", levels))
            _same_bits(out.cpu().numpy(), c.astype(np.float32) / np.float32(256), ("mask", levels))
            want = ref.pyramid((c >= 128).astype(np.uint8), levels, ref.down_mask)
            for lv, g in enumerate(_levels_of(mp, H, W, levels)):
                _same(g[0], want[lv], ("next bits", levels, lv))
    assert filled


@stage
def test_visible_flags_and_occlude_under_poison(poison, monkeypatch):
    filled = poisoned_empty(monkeypatch, poison)
    Yt, Yk = inputs._visible_lumas("noisy", H, W)
    for positions in ("smooth", "outside"):
        P = inputs._positions(positions, H, W)
        for name in ("disc", "sparse"):
            m = inputs.VISIBLE_MASKS[name](H, W)
            want = vref.visible_flags(Yt, Yk, P, m, 16)
            got = propagate_visible.visible_flags(_dev(P.astype(np.int32)), _dev(Yt), _dev(Yk), _dev(m), 16)
            _same(got.cpu().numpy(), want, ("flags", positions, name))
    flags = inputs._flags("random", *ref.grid_of(H, W))
    c = _rng(H, W, 12).integers(0, 257, (H, W))
    cv = vref.occlude(c, flags)
    for levels in (1, 4):
        out, hidden, mpyr = propagate_visible.occlude(_dev((c / 256).astype(np.float32)), _dev(flags.astype(np.int32)), levels)
        _same_bits(out.cpu().numpy(), cv.astype(np.float32) / np.float32(256), "mask")
        _same_bits(hidden.cpu().numpy(), (c - cv).astype(np.float32) / np.float32(256), "hidden")
        want = ref.pyramid((cv >= 128).astype(np.uint8), levels, ref.down_mask)
        for lv, g in enumerate(_levels_of(mpyr, H, W, levels)):
            _same(g[0], want[lv], ("next bits", levels, lv))
    assert filled


@stage
def test_anchor_field_under_poison(poison, monkeypatch):
    filled = poisoned_empty(monkeypatch, poison)
    for positions, lumas, mask in (("smooth", "noisy", "disc"), ("outside", "flat", "random"), ("key", "noisy", "empty")):
        P, Yt, Yk, m = inputs._anchored_inputs(SMALL, positions, lumas, mask)
        want_vec, want_valid = aref.anchor_field(P, Yt, Yk, m, 2, SMOOTH)
        vec, valid = motion_checks._anchored_field(P, Yt, Yk, m, 2, SMOOTH)
        _same(valid, want_valid, ("valid", positions, lumas, mask))
        _same(vec, want_vec, ("vec", positions, lumas, mask))
    assert filled


@stage
def test_the_batched_step_entries_under_poison(poison, monkeypatch):
    """match_level_batch, fill_median_batch and advance_batch against the single entries, which the test above holds to the
    restatement under the same poison: the suite's own test, on this plane."""
    filled = poisoned_empty(monkeypatch, poison)
    motion_checks._check_batched_entries(SMALL, 5)
    assert filled


@stage
def test_visible_flags_batch_and_occlude_batch_under_poison(poison, monkeypatch):
    filled = poisoned_empty(monkeypatch, poison)
    jobs = 5
    made = [inputs._visible_job(H, W, j) for j in range(jobs)]
    got = propagate_keys_visible.visible_flags_batch([(_dev(P.astype(np.int32)), _dev(Yt), _dev(Yk), _dev(m)) for P, Yt, Yk, m in made], 16)
    for j, (P, Yt, Yk, m) in enumerate(made):
        _same(got[j].cpu().numpy(), vref.visible_flags(Yt, Yk, P, m, 16), ("flags", j))
    made = [inputs._occlude_job(H, W, j) for j in range(jobs)]
    feed = [(_dev((c / 256).astype(np.float32)), _dev(flags.astype(np.int32))) for c, flags in made]
    counts = torch.arange(jobs, dtype=torch.int32, device=feed[0][0].device) * 3       # added to, not overwritten
    got = propagate_keys_visible.occlude_batch(feed, 4, counts)
    for j, (c, flags) in enumerate(made):
        cv = vref.occlude(c, flags)
        out, hidden, mpyr = got[j]
        _same_bits(out.cpu().numpy(), cv.astype(np.float32) / np.float32(256), ("mask", j))
        _same_bits(hidden.cpu().numpy(), (c - cv).astype(np.float32) / np.float32(256), ("hidden", j))
        want = ref.pyramid((cv >= 128).astype(np.uint8), 4, ref.down_mask)
        for lv, g in enumerate(_levels_of(mpyr, H, W, 4)):
            _same(g[0], want[lv], ("next bits", j, lv))
    _same(counts.cpu().numpy(), [3 * j + int((vref.occlude(c, flags) >= 128).sum()) for j, (c, flags) in enumerate(made)], "counts")
    assert filled


@stage
def test_merge_gap_and_merge_gap_visible_under_poison(poison, monkeypatch):
    filled = poisoned_empty(monkeypatch, poison)
    span = 3
    pairs = np.array([(a, b) for a in inputs.KEYS_SPECIAL for b in inputs.KEYS_SPECIAL], dtype=np.int64)
    rng = _rng(span, H, W, 2, 1)
    q = rng.integers(-5000, 5001, (2, 2, H, W))
    q[q == 0] = 1
    pick = rng.random((2, H, W)) < 0.6
    chosen = pairs[rng.integers(0, len(pairs), (2, H, W))]
    q[0][pick], q[1][pick] = chosen[..., 0][pick], chosen[..., 1][pick]
    got = propagate_keys.merge_gap(_dev(q[0].astype(np.int32)), _dev(q[1].astype(np.int32)), span, 1).cpu().numpy()
    _same_bits(got, np.stack([kref.merge(q[0][f], q[1][f], span, 1 + f) for f in range(2)]), "merge")
    q, c, cv, f = motion_checks._merge_inputs(H, W, span, "random")
    dq, dc, dcv, df = (_dev(q.astype(np.int32)), _dev((c / 256).astype(np.float32)), _dev((cv / 256).astype(np.float32)),
                       _dev(f.astype(np.int32)))
    for kind in ("none_lost", "a_lost", "both_lost"):
        na, nb = inputs._counts(kind, span)
        want, want_hidden = inputs._merge_want(q, c, cv, f, na, nb, span)
        out, hidden = propagate_keys_visible.merge_gap_visible(dq[0], dq[1], dc[0], dcv[0], dc[1], dcv[1], df[0], df[1],
                                                               _dev(np.array(na, np.int32)), _dev(np.array(nb, np.int32)), span)
        _same_bits(out.cpu().numpy(), want, ("mask", kind))
        _same_bits(hidden.cpu().numpy(), want_hidden, ("hidden", kind))
    assert filled


@stage
def test_step_fields_under_poison(poison, monkeypatch):
    """34 steps of 18 frames, two launches a level: against the single entries and the restatement, the suite's own test."""
    filled = poisoned_empty(monkeypatch, poison)
    motion_checks._check_batched_fields()
    assert filled


@stage
def test_shot_scores_and_shot_decide_under_poison(poison, monkeypatch):
    filled = poisoned_empty(monkeypatch, poison)
    images = _video(F, H, W, 3)
    for level, search in ((0, 1), (2, 2), (5, 3)):
        motion_checks._check_scores(images, level, search, (level, search))
    score = inputs._random_scores(257, 1000, 0)
    for window, ratio, threshold, hist in ((1, 100, 16, 30), (4, 200, 1, 0)):
        want = shref.shot_decide(score, 1000, threshold, hist, ratio, window)
        assert want[-1] > 0
        _same(shots.shot_decide(_dev(score), 1000, threshold, hist, ratio, window).cpu().numpy(), want, (window, ratio, threshold, hist))
    assert filled


# ---- C: off the default stream, behind a delay ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("call", CALLS)
def test_the_call_on_a_held_back_side_stream_reads_nothing_back(call, monkeypatch):
    """The call is made on a side stream that is still busy with a delay queued in front of it.  The delay's event is not done
    when the call returns: so the call neither read from the device nor synchronised a stream or the device (the docstrings' "no
    device -> host read"), and the delay did outlast the host's side of the call -- were it too short, this fails rather than
    proving nothing.  Every launch, copy and memset the call makes has to wait on that stream behind the poison fills of its
    buffers; one that went to the null stream runs ahead of its producers and reads poison, or is overwritten by the poison
    queued behind the delay, and either way the bits differ from the restatement's.  Unless the runtime happens to have put the
    null stream and the side stream on one hardware queue: then the stray operation waits behind the delay too, in the order it
    was issued, and computes the right bits -- but it is still pending on the null stream when the call returns, and the null
    stream, on which nothing was queued since the inputs were built and waited for, is asked whether it is idle."""
    levels, mode = 3, "whole"
    want = _want(call, SMALL, levels, mode)
    args = _device_inputs(SMALL, mode)                                 # built on the default stream
    cycles = int(_spin_cycles_per_ms() * DELAY_MS)
    torch.cuda.synchronize()
    filled = poisoned_empty(monkeypatch, 0xFF)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        _run(call, levels, *args)                                      # the first call loads the kernels and fills the allocator's
        side.synchronize()                                             # pool of this stream: no hipMalloc below
        start = time.perf_counter()
        warm = _run(call, levels, *args)
        warm_ms = (time.perf_counter() - start) * 1e3
        del warm
        side.synchronize()
        del filled[:]
        done = torch.cuda.Event()
        torch.cuda._sleep(cycles)
        done.record(side)
        start = time.perf_counter()
        got = _run(call, levels, *args)
        held = not done.query()                                        # directly behind the call, before anything synchronises
        idle = torch.cuda.default_stream().query()
        call_ms = (time.perf_counter() - start) * 1e3
    print(f"{call}: warm call {warm_ms:.2f} ms, call behind the delay {call_ms:.2f} ms of host time; delay {DELAY_MS} ms")
    assert held, (f"{call} returned after {call_ms:.2f} ms with the {DELAY_MS} ms delay in front of it done: it waited for the device, "
                  "or the delay is too short for this host")
    assert idle, f"{call} left work on the null stream"
    assert filled
    side.synchronize()
    _compare(call, got, want, (call, "side stream"))
