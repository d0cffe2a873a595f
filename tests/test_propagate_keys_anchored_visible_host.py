"""The anchored occlusion-aware video mask propagate from several keyframes, the parts that need no device: the restatement
(tests/propagate_keys_anchored_visible_ref.py) against the restatements of the seven existing forms and on the clips the form is
for, the gated form of lp_prop_match_batch's argument checks (made before any HIP call), `propagate_keys.Chains` with both
options on host memory with its launches recorded, the wrapper's, the nodes' and the per-shot form's checks and protocol.  The
macro against the header as gcc reads it is tests/test_cabi_mirror.py's, with the whole C ABI.

A descriptor that the library would accept is never handed over here: its addresses are made up, and on a machine with a device
the launch would follow them.  That the gated form accepts what it should is tests/test_gpu_propagate_keys_anchored_visible.py's,
on real buffers."""
import ctypes
import os

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, _motion, propagate_keys
from tests import propagate_anchored_visible_ref as avref
from tests import propagate_keys_anchored_ref as karef
from tests import propagate_keys_anchored_visible_ref as kavref
from tests import propagate_keys_ref as kref
from tests import propagate_keys_visible_ref as kvref
from tests import propagate_ref as ref
from tests.compare import _f32_bits as _bits
from tests.device import _match_jobs as _jobs
from tests.propagate_scenes import (_moving, _moving_disc as _disc, assert_the_keys_quality_lines as assert_the_quality_lines,
                                    keys_quality_case as quality_case)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATED = _cabi.LP_PROP_MATCH_GATED
LEVELS, SEARCH, SMOOTH, ANCHOR, OCCLUSION = 3, 2, 8, 2, 16


def _same(got, want, what):
    for g, w, name in zip(got, want, ("mask", "hidden")):
        assert g.dtype == np.float32 and (_bits(g) == _bits(w)).all(), (what, name)


# ---- what follows from the rule, on the restatement alone -----------------------------------------------------------------------------------
def test_one_key_is_the_single_key_anchored_visible_chain_and_so_is_a_frame_outside_the_keys():
    H, W, F = 23, 33, 6
    video = _moving(F, H, W)                                            # a static bar in front: flags and gates do fire
    soft = np.random.default_rng(2).random((H, W), dtype=np.float32)
    fired = 0
    for key in (0, 2, 5):
        for anchor, occlusion in ((1, 16), (2, 4)):
            got = kavref.propagate_keys_anchored_visible_ref(video, soft[None], [key], LEVELS, SEARCH, SMOOTH, anchor, occlusion)
            want = avref.propagate_anchored_visible_ref(video, soft, key, LEVELS, SEARCH, SMOOTH, anchor, occlusion)
            _same(got, want, (key, anchor, occlusion))
            fired += int(want[1].any())
    assert fired                                                       # not on zero hidden parts only
    masks = np.stack([soft, _disc(H, W, 11, 16, 7)])
    got = kavref.propagate_keys_anchored_visible_ref(video, masks, [1, 4], LEVELS, SEARCH, SMOOTH, ANCHOR, OCCLUSION)
    first = avref.propagate_anchored_visible_ref(video, masks[0], 1, LEVELS, SEARCH, SMOOTH, ANCHOR, OCCLUSION)
    last = avref.propagate_anchored_visible_ref(video, masks[1], 4, LEVELS, SEARCH, SMOOTH, ANCHOR, OCCLUSION)
    _same([p[0] for p in got], [p[0] for p in first], "in front of the first key")
    _same([p[5] for p in got], [p[5] for p in last], "behind the last key")


def test_the_three_off_routes():
    H, W, F = 23, 33, 6
    video = _moving(F, H, W)
    masks = np.stack([np.random.default_rng(2).random((H, W), dtype=np.float32), _disc(H, W, 11, 16, 7)])
    zeros = np.zeros((F, H, W), np.float32)
    for anchor, occlusion, want in ((0, 16, kvref.propagate_keys_visible_ref(video, masks, [1, 4], LEVELS, SEARCH, SMOOTH, 16)),
                                    (2, 0, (karef.propagate_keys_anchored_ref(video, masks, [1, 4], LEVELS, SEARCH, SMOOTH, 2), zeros)),
                                    (0, 0, (kref.propagate_keys_ref(video, masks, [1, 4], LEVELS, SEARCH, SMOOTH), zeros))):
        _same(kavref.propagate_keys_anchored_visible_ref(video, masks, [1, 4], LEVELS, SEARCH, SMOOTH, anchor, occlusion), want,
              (anchor, occlusion))
    on = kavref.propagate_keys_anchored_visible_ref(video, masks, [1, 4], LEVELS, SEARCH, SMOOTH, 2, 16)
    assert (_bits(on[0]) != _bits(kvref.propagate_keys_visible_ref(video, masks, [1, 4], LEVELS, SEARCH, SMOOTH, 16)[0])).any()


def test_a_still_video_empty_keys_the_keys_themselves_and_the_codes():
    rng = np.random.default_rng(3)
    H, W, F = 23, 33, 6
    soft = rng.random((H, W), dtype=np.float32)
    binar = ref.binarise(soft).astype(np.float32)
    still = np.repeat(rng.random((1, H, W, 3), dtype=np.float32), F, axis=0)
    for keys in ([0, 5], [1, 3, 4], [2]):
        for anchor, occlusion in ((2, 1), (2, 16), (7, 255)):
            mask, hidden = kavref.propagate_keys_anchored_visible_ref(still, np.repeat(soft[None], len(keys), axis=0), keys, LEVELS,
                                                                      SEARCH, SMOOTH, anchor, occlusion)
            assert mask.dtype == hidden.dtype == np.float32
            assert (_bits(mask) == _bits(np.repeat(binar[None], F, axis=0))).all() and (_bits(hidden) == 0).all(), (keys, anchor, occlusion)
    video = _moving(F, H, W)
    mask, hidden = kavref.propagate_keys_anchored_visible_ref(video, np.zeros((3, H, W), np.float32), [0, 3, 5], LEVELS, SEARCH, SMOOTH, 7, 1)
    assert (_bits(mask) == 0).all() and (_bits(hidden) == 0).all()
    # on every key the painting and a zero hidden; mask + hidden a multiple of 1 / 256 everywhere, at a threshold that flags a lot
    masks = np.stack([_disc(H, W, 11, 10, 7), soft, _disc(H, W, 12, 20, 6)])
    for occlusion in (1, 16):
        mask, hidden = kavref.propagate_keys_anchored_visible_ref(video, masks, [0, 3, 5], LEVELS, SEARCH, SMOOTH, ANCHOR, occlusion)
        for i, k in enumerate((0, 3, 5)):
            assert (_bits(mask[k]) == _bits(ref.binarise(masks[i]).astype(np.float32))).all() and (_bits(hidden[k]) == 0).all()
        total = (mask.astype(np.float64) + hidden.astype(np.float64)) * 256
        assert (total == np.round(total)).all() and total.min() >= 0 and total.max() <= 256
        assert (mask >= 0).all() and (hidden >= 0).all()
        assert occlusion != 1 or hidden.sum() > 0


# ---- the quality lines ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "disc"])
def test_the_new_form_holds_where_either_several_keys_form_fails(name):
    _, masks, keys, _, truth, new, trace, keys_visible, keys_anchored = quality_case(name)
    figures = assert_the_quality_lines(name, truth, new, keys_visible, keys_anchored)
    want = {"A": (0.910, 0.956, 0.770, 0.873, 0.781, 0.874), "B": (0.894, 0.941, 0.669, 0.825, 0.807, 0.881),
            "disc": (0.837, 0.946, 0.921, 0.967, 0.000, 0.243)}[name]
    assert tuple(round(v, 3) for v in figures) == want
    for i, k in enumerate(keys):                                       # a key frame returns its painting and a zero hidden
        assert (_bits(new[0][k]) == _bits(masks[i])).all() and not new[1][k].any()
    if name == "disc":                                                 # the lost-chain recovery is the keys-visible form's
        lost = trace["lost"]
        assert sorted(lost) == list(range(1, 15))
        assert sum(1 for a, b in lost.values() if a != b) == 13 and lost[7] == (True, True)
        assert [t for t in lost if lost[t][0]] == list(range(7, 15)) and [t for t in lost if lost[t][1]] == list(range(1, 8))


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
FIELDS = [f for f, _ in _cabi.LpPropMatchJob._fields_]


def test_the_gated_form_rejects_bad_arguments_without_a_device(hip_lib):
    C, E, J = ctypes, _cabi.LP_E_INVALID, _cabi.LP_PROP_MAX_JOBS
    side = _cabi.LP_VMASK_MAX_SIDE
    a = [256 * (i + 1) for i in range(8)]                             # never dereferenced: every descriptor here is refused
    good_job = (a[0], a[1], a[2], a[3], a[4], a[5])
    keep, ptr = _jobs([good_job] * J)
    good = dict(height=40, width=70, levels=3, level=0, search=2, smooth=8, jobs=2, reserved0=GATED(16), job=ptr)
    assert GATED(16) == 1 | (16 << 8) == 4097 and GATED(1) == 257 and GATED(255) == 0xFF01

    def call(**change):
        return hip_lib.lp_prop_match_batch(C.byref(_cabi.LpPropMatchBatchDesc(**{**good, **change})), None)
    for change in ({"level": 1}, {"level": 2}, {"level": -1}, {"levels": 1, "level": 1}, {"search": 0}, {"search": 8}, {"search": -1},
                   {"smooth": -1}, {"smooth": 65}, {"height": 0}, {"width": side + 1}, {"levels": 0}, {"levels": 7}, {"jobs": 0},
                   {"jobs": J + 1}, {"job": None}):
        assert call(**change) == E, change
    stray = [1 | (1 << bit) for bit in range(1, 8)] + [GATED(16) | (1 << bit) for bit in range(1, 8)]        # bits 1..7
    high = [GATED(16) | (1 << bit) for bit in range(16, 31)] + [GATED(16) - (1 << 31), 1 | (1 << 16), 1 - (1 << 31)]   # bits 16..31
    no_source = [16 << 8, 255 << 8, (16 << 8) | 2]                     # an occlusion without the warped-key bit
    for value in stray + high + no_source + [2, 3, -1, 1 << 16, -(1 << 31)]:
        assert call(reserved0=value) == E, value
        assert call(reserved0=value, level=1) == E, value
    for at in (0, 1, J - 1):                                          # one bad job anywhere in the table: the warped form's list
        bad = [(f, None) for f in FIELDS]                              # a null pointer, the positions in `parent` included
        bad += [(out, a[FIELDS.index(inp)]) for out in ("vec", "valid") for inp in ("src", "tgt", "mask", "parent")]
        bad += [("vec", a[5]), ("valid", a[4])]                        # the two outputs on one another
        for levels, occlusion in ((1, 1), (3, 16), (3, 255)):          # a null parent is refused at levels 1 too: it is P_t
            for field, value in bad:
                rows = [list(good_job) for _ in range(J)]
                rows[at][FIELDS.index(field)] = value
                keep2, ptr2 = _jobs(rows)
                assert call(levels=levels, jobs=at + 1, job=ptr2, reserved0=GATED(occlusion)) == E, (at, levels, field, value)


def test_no_new_entry_and_the_words_are_everywhere():
    assert len([n for n in _cabi.EXPORTS if n.startswith("lp_prop_")]) == 17                       # no new entry
    assert not [n for n in _cabi.EXPORTS if "keys_anchored" in n or "gated_batch" in n]
    header = open(os.path.join(ROOT, "include", "lanpaint_hip.h")).read()
    for word in ("Video mask propagate from several keys, anchored and occlusion-aware", "#define LP_PROP_MATCH_GATED(occlusion)",
                 "every chain is the anchored occlusion-aware chain of its own", "writes that plane only where its pointer is non-null",
                 "2 L + 6 launches", "Not handled: occlusion.", "several keys", "re-anchoring every n-th frame only"):
        assert word in header, word
    assert "re-anchoring against drift" not in header
    for doc in ("README.md", "DESIGN.md", "CHANGES.md", "INTEGRATION.md"):
        assert "LanPaint_VideoMaskPropagateKeysAnchoredVisible" in open(os.path.join(ROOT, doc)).read(), doc
    from lanpaint_amd import propagate_anchored, propagate_anchored_visible, propagate_keys_anchored, propagate_keys_visible
    for module in (propagate_anchored, propagate_anchored_visible, propagate_keys_anchored, propagate_keys_visible):
        assert "propagate_keys_anchored_visible.py" in module.__doc__, module.__name__


# ---- the chain table with both options on -----------------------------------------------------------------------------------------------------
def test_the_chains_tables_with_both_options(monkeypatch):
    """`propagate_keys.Chains(..., split=..., rematch=(2, 16))` on host memory, its launches recorded: 6 frames with keys on 1 and 4,
    so an edge chain backwards of 1 step, the gap's forward and backward chains of 2 steps and an edge chain forwards of 1 step.
    For steps 1 and 2: the entries in order, each descriptor's numbers, `jobs` and source form, and every row of every table
    against addresses worked out by hand from the buffers' `data_ptr()` and row sizes; and the option's three refusals."""
    H, W, levels, search, smooth, anchor, occlusion, F = 20, 12, 2, 3, 5, 2, 16, 6
    plan = propagate_keys.chain_plan(F, [1, 4])
    assert plan == [(0, 1, -1, 1), (0, 1, 1, 2), (1, 4, -1, 2), (1, 4, 1, 1)]
    stride = _cabi.prop_pyramid_ws_bytes(1, H, W, levels)
    plane, cells, positions = H * W * 4, 3 * 2 * 4, H * W * 2 * 4      # fp32 [H, W], int32 [3, 2], int32 [H, W, 2]: bytes a row
    f32, i32, u8 = torch.float32, torch.int32, torch.uint8
    pyr = torch.zeros((F, stride), dtype=u8)
    key_pyrs = [torch.zeros((1, stride), dtype=u8) for _ in range(2)]
    out, hidden, scratch = torch.zeros((F, H, W), dtype=f32), torch.zeros((F, H, W), dtype=f32), torch.zeros((4, H, W), dtype=f32)
    back, flags = torch.zeros((2, 2, H, W), dtype=f32), torch.zeros((2, 2, 3, 2), dtype=i32)
    scratch_flags, counts = torch.zeros((5, 3, 2), dtype=i32), torch.zeros(6, dtype=i32)
    at = lambda t: t.data_ptr()                                        # noqa: E731
    # as tests/test_motion_host.py lays the occlusion-aware option out: per chain (address, byte step)
    code = [(at(scratch[0]), 0), (at(hidden) + plane, plane), (at(back[0]) + 2 * plane, -plane), (at(scratch[3]), 0)]
    mask = [(at(out) + plane, -plane), (at(out) + plane, plane), (at(back[1]) + 2 * plane, -plane), (at(out) + 4 * plane, plane)]
    hid = [(at(hidden) + plane, -plane), (at(scratch[1]), 0), (at(scratch[2]), 0), (at(hidden) + 4 * plane, plane)]
    flag = [(at(scratch_flags[0]), 0), (at(flags[0]) - cells, cells), (at(flags[1]) + 2 * cells, -cells), (at(scratch_flags[3]), 0)]
    count = [(0, 0), (at(counts), 4), (at(counts) + 3 * 4, 4), (0, 0)]
    split = (occlusion, mask, hid, flag, count)
    columns = {"lp_prop_match_batch": 6, "lp_prop_fill_batch": 3, "lp_prop_advance_batch": 6, "lp_prop_visible_batch": 5,
               "lp_prop_occlude_batch": 6}
    launched = []

    def record(entry, dev, *args):
        if entry == "lp_prop_fill_batch":
            table, jobs, *numbers = args
        else:
            d = args[0]._obj
            table, jobs = d.job, d.jobs
            numbers = [getattr(d, name) for name, _ in d._fields_ if name not in ("jobs", "job")]
        rows = np.ctypeslib.as_array((ctypes.c_uint64 * (jobs * columns[entry])).from_address(table)).reshape(jobs, columns[entry])
        launched.append((entry, numbers, rows.tolist()))
    for module in (_motion, propagate_keys):
        monkeypatch.setattr(module, "launch", record)

    make = lambda **kw: propagate_keys.Chains(plan, pyr, key_pyrs, code, H, W, levels, search, smooth, **kw)    # noqa: E731
    with pytest.raises(ValueError, match="rematch with split"):        # the ungated re-match next to the split: as it was
        make(split=split, rematch=(anchor,))
    with pytest.raises(ValueError, match="without split"):             # the gated re-match has nothing to gate for
        make(rematch=(anchor, occlusion))
    with pytest.raises(ValueError, match="is not split's"):            # one occlusion a chain
        make(split=split, rematch=(anchor, occlusion + 1))
    for bad in ((0, 16), (8, 16), (2.0, 16), (True, 16), (2, 0), (2, 256), (2, 16.0), (2, True), (2, 16, 0)):
        with pytest.raises(ValueError):
            make(split=(bad[1], mask, hid, flag, count) if len(bad) == 2 else split, rematch=bad)
    chains = make(split=split, rematch=(anchor, occlusion))

    # no buffer beyond the two options': the split's raw_mpyr serves both advances
    assert [(tuple(t.shape), t.dtype) for t in chains._keep] == [((4, H, W, 2), i32)] * 2 + [((4, stride), u8)] * 3 + [((4, H, W, 2), i32)]
    pos, mpyr, raw_mpyr, raw_pos = chains._keep[0:2], chains._keep[2:4], chains._keep[4], chains._keep[5]
    raw0, valid0, field0, raw1, valid1, field1 = chains.walk._keep
    assert [tuple(t.shape) for t in chains.walk._keep] == [(4, 3, 2, 2), (4, 3, 2), (4, 3, 2, 2), (4, 2, 1, 2), (4, 2, 1), (4, 2, 1, 2)]

    def want_step(s, active):
        """The launches of step s for the chains `active` of the plan: chain c is row j of every table."""
        rows = {name: [] for name in ("match1", "fill1", "match0", "fill0", "first", "rematch", "second", "visible", "occlude")}
        for j, c in enumerate(active):
            i, k, d, _ = plan[c]
            src, tgt = at(pyr) + (k + d * (s - 1)) * stride, at(pyr) + (k + d * s) * stride
            weight = at(key_pyrs[i]) if s == 1 else at(mpyr[(s - 1) & 1]) + c * stride
            pos_src = 0 if s == 1 else at(pos[(s - 1) & 1]) + c * positions
            pos_t, mpyr_t = at(pos[s & 1]) + c * positions, at(mpyr[s & 1]) + c * stride
            raw_pos_t, bits = at(raw_pos) + c * positions, at(raw_mpyr) + c * stride       # the chain's, not the group's
            r1, v1, f1 = at(raw1) + j * 16, at(valid1) + j * 8, at(field1) + j * 16      # the walk's rows are the group's
            r0, v0, f0 = at(raw0) + j * 48, at(valid0) + j * 24, at(field0) + j * 48
            written = code[c][0] + s * code[c][1]                      # the code: both advances write it
            mask_t, hidden_t, flags_t, count_t = (col[c][0] + s * col[c][1] for col in split[1:])
            key_luma = at(pyr) + k * stride
            rows["match1"].append([src, tgt, weight, 0, r1, v1])
            rows["fill1"].append([r1, v1, f1])
            rows["match0"].append([src, tgt, weight, f1, r0, v0])
            rows["fill0"].append([r0, v0, f0])
            rows["first"].append([f0, pos_src, at(key_pyrs[i]), raw_pos_t, written, bits])
            rows["rematch"].append([key_luma, tgt, bits, raw_pos_t, r0, v0])
            rows["second"].append([f0, raw_pos_t, at(key_pyrs[i]), pos_t, written, bits])
            rows["visible"].append([pos_t, tgt, key_luma, bits, flags_t])
            rows["occlude"].append([written, flags_t, mask_t, hidden_t, mpyr_t, count_t])
        return [("lp_prop_match_batch", [H, W, levels, 1, search, smooth, 0], rows["match1"]), ("lp_prop_fill_batch", [2, 1], rows["fill1"]),
                ("lp_prop_match_batch", [H, W, levels, 0, search, smooth, 0], rows["match0"]), ("lp_prop_fill_batch", [3, 2], rows["fill0"]),
                ("lp_prop_advance_batch", [H, W, levels], rows["first"]),
                ("lp_prop_match_batch", [H, W, levels, 0, anchor, smooth, GATED(occlusion)], rows["rematch"]),
                ("lp_prop_fill_batch", [3, 2], rows["fill0"]),
                ("lp_prop_advance_batch", [H, W, levels], rows["second"]),
                ("lp_prop_visible_batch", [H, W, occlusion], rows["visible"]),
                ("lp_prop_occlude_batch", [H, W, levels], rows["occlude"])]

    painted, zero_flags = [out[k] for _, k, _, _ in plan], scratch_flags[4]
    chains.count_keys(painted, zero_flags)                             # as with the split alone: scribbles on pos[0], mpyr[0], hidden
    assert launched == [("lp_prop_occlude_batch", [H, W, levels], [
        [at(painted[c]), at(zero_flags), at(pos[0]) + c * positions, at(scratch[c]), at(mpyr[0]) + c * stride, count[c][0]] for c in (1, 2)])]
    del launched[:]
    chains.step(1)
    assert len(launched) == 2 * levels + 6
    assert launched == want_step(1, [0, 1, 2, 3])
    assert all(row[1] == 0 for row in launched[4][2])                  # a null pos_src: the key frame's positions
    touched = {row[col] for entry in (4, 7) for row in launched[entry][2] for col in (3, 5)}       # what step 1's advances write
    assert not touched & {at(pos[0]) + c * positions for c in range(4)} and not touched & {at(mpyr[0]) + c * stride for c in range(4)}
    assert [row[0] for row in launched[5][2]] == [at(pyr) + k * stride for k in (1, 1, 4, 4)]      # each chain's own key frame
    del launched[:]
    chains.step(2)
    assert launched == want_step(2, [1, 2]) and all(len(rows) == 2 for _, _, rows in launched)
    assert [row[1] for row in launched[4][2]] == [at(pos[1]) + c * positions for c in (1, 2)]       # read what step 1's second
    assert [row[3] for row in launched[7][2]] == [at(pos[0]) + c * positions for c in (1, 2)]       # advance wrote, write the other
    assert [row[2] for row in launched[0][2]] == [at(mpyr[1]) + c * stride for c in (1, 2)]         # occlude's visible bits weigh
    assert [row[2] for row in launched[9][2]] == [at(out[3]), at(back[1][0])]                       # frame 3, and frame 2 in the stack
    assert [row[5] for row in launched[9][2]] == [at(counts) + 8, at(counts) + 20]                  # N at step 2 of either chain
    del launched[:]
    chains.step(3)
    assert launched == []


def test_either_option_alone_allocates_and_launches_what_it_did(monkeypatch):
    H, W, levels, F = 20, 12, 2, 6
    plan = propagate_keys.chain_plan(F, [1, 4])
    stride = _cabi.prop_pyramid_ws_bytes(1, H, W, levels)
    pyr, key_pyrs = torch.zeros((F, stride), dtype=torch.uint8), [torch.zeros((1, stride), dtype=torch.uint8) for _ in range(2)]
    out = torch.zeros((F, H, W), dtype=torch.float32)
    outs = [(out.data_ptr(), 0)] * 4
    names = []
    for module in (_motion, propagate_keys):
        monkeypatch.setattr(module, "launch", lambda entry, *a: names.append(entry))
    walk = ["lp_prop_match_batch", "lp_prop_fill_batch"] * levels
    for kw, buffers, tail in (({}, 4, ["lp_prop_advance_batch"]),
                              ({"split": (16, outs, outs, outs, outs)}, 5, ["lp_prop_advance_batch", "lp_prop_visible_batch", "lp_prop_occlude_batch"]),
                              ({"rematch": (2,)}, 6, ["lp_prop_advance_batch", "lp_prop_match_batch", "lp_prop_fill_batch", "lp_prop_advance_batch"])):
        chains = propagate_keys.Chains(plan, pyr, key_pyrs, outs, H, W, levels, 3, 5, **kw)
        assert len(chains._keep) == buffers, kw
        del names[:]
        chains.step(1)
        assert names == walk + tail, kw


# ---- the wrappers, the nodes and the per-shot form ----------------------------------------------------------------------------------------------
def test_propagate_keys_anchored_visible_refuses_cpu_tensors_and_bad_arguments():
    from lanpaint_amd import propagate_keys_anchored_visible as pkav
    images, masks = torch.zeros(7, 16, 16, 3), torch.zeros(2, 16, 16)
    for anchor, occlusion in ((2, 16), (0, 16), (2, 0), (0, 0)):       # every route
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pkav.propagate_keys_anchored_visible(images, masks, [0, 6], anchor=anchor, occlusion=occlusion)
    row = torch.zeros(_cabi.prop_pyramid_ws_bytes(1, 16, 16, 3), dtype=torch.uint8)
    positions = torch.zeros(16, 16, 2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkav.anchor_field_batch([(row, row, row, positions)], 16, 16, 3, 2, 8, 16)
    assert pkav.anchor_field_batch is propagate_keys.anchor_field_batch
    for bad in (dict(occlusion=-1), dict(occlusion=256), dict(occlusion=16.0), dict(occlusion=True), dict(anchor=0), dict(anchor=8)):
        with pytest.raises(ValueError):
            pkav.anchor_field_batch([(row, row, row, positions)], 16, 16, **{"levels": 3, "anchor": 2, "smooth": 8, "occlusion": 16, **bad})
    # the numbers are checked before the tensors are looked at
    for bad in (dict(levels=0), dict(levels=7), dict(search=0), dict(search=8), dict(smooth=-1), dict(smooth=65), dict(anchor=-1),
                dict(anchor=8), dict(anchor=2.0), dict(anchor=True), dict(anchor=None), dict(occlusion=-1), dict(occlusion=256),
                dict(occlusion=16.0), dict(occlusion=None)):
        with pytest.raises(ValueError):
            pkav.propagate_keys_anchored_visible(images, masks, [0, 6], **bad)
    for keys in ([], [6, 0], [0, 0], [0, 7], [-1, 3], [0.0, 6], None, 3):
        for anchor, occlusion in ((2, 16), (0, 16), (2, 0)):
            with pytest.raises(ValueError):
                pkav.propagate_keys_anchored_visible(images, masks, keys, anchor=anchor, occlusion=occlusion)
    assert (pkav.DEFAULT_ANCHOR, pkav.MAX_ANCHOR, pkav.DEFAULT_OCCLUSION, pkav.MAX_OCCLUSION, pkav.WS_CAP_BYTES) == (2, 7, 16, 255, 1 << 30)
    doc = " ".join(pkav.__doc__.split())
    for word in ("Not handled: following a subject through a full occlusion", "what leaves the picture", "occlusion edges finer than a block",
                 "a subject whose look changes", "no CPU fallback", "2 levels + 6 launches"):
        assert word in doc, word


def test_keys_anchored_visible_node_protocol_and_own_mappings():
    from lanpaint_amd import propagate_anchored_visible_nodes, propagate_keys_anchored_nodes, propagate_keys_nodes, shots_nodes
    from lanpaint_amd import propagate_keys_anchored_visible_nodes as nodes
    node, per_shot = nodes.LanPaint_VideoMaskPropagateKeysAnchoredVisible, nodes.LanPaint_VideoMaskPropagateKeysAnchoredVisibleShots
    assert nodes.NODE_CLASS_MAPPINGS == {"LanPaint_VideoMaskPropagateKeysAnchoredVisible": node,
                                         "LanPaint_VideoMaskPropagateKeysAnchoredVisibleShots": per_shot}
    assert nodes.NODE_DISPLAY_NAME_MAPPINGS == {
        "LanPaint_VideoMaskPropagateKeysAnchoredVisible": "LanPaint Video Mask Propagate (Keys, Anchored, Visible)",
        "LanPaint_VideoMaskPropagateKeysAnchoredVisibleShots": "LanPaint Video Mask Propagate (Keys, Anchored, Visible, Shots)"}
    types = node.INPUT_TYPES()
    req = types["required"]
    assert list(types) == ["required"]
    assert list(req) == ["image", "mask", "key_frames", "levels", "search", "smooth", "anchor", "occlusion"]
    keys_req = propagate_keys_nodes.LanPaint_VideoMaskPropagateKeys.INPUT_TYPES()["required"]
    for name in ("image", "mask", "key_frames", "levels", "search", "smooth"):
        assert req[name] == keys_req[name], name
    assert req["anchor"] == propagate_keys_anchored_nodes.LanPaint_VideoMaskPropagateKeysAnchored.INPUT_TYPES()["required"]["anchor"]
    assert req["occlusion"] == propagate_anchored_visible_nodes.LanPaint_VideoMaskPropagateAnchoredVisible.INPUT_TYPES()["required"]["occlusion"]
    assert req["anchor"][1] == {**req["anchor"][1], "default": 2, "min": 0, "max": 7}
    assert req["occlusion"][1] == {**req["occlusion"][1], "default": 16, "min": 0, "max": 255}
    for name in req:
        assert len(req[name][1]["tooltip"]) > 20, name
    assert node.RETURN_TYPES == ("MASK", "MASK") and node.RETURN_NAMES == ("mask", "hidden") and len(node.OUTPUT_TOOLTIPS) == 2
    assert node.FUNCTION == "propagate" and node.CATEGORY == "mask" and callable(getattr(node, node.FUNCTION))
    for word in ("key frames", "motion", "merged", "key frame again", "long gap", "in front of the subject", "`hidden`",
                 "second key behind the occluder", "stabilize", "mask refine", "encode", "Detailer", "empty key", "full occlusion",
                 "leaves the picture", "finer than a block", "look changes"):
        assert word in node.DESCRIPTION, word
    assert issubclass(per_shot, node) and per_shot.__mro__[1] is shots_nodes._PerShot
    assert per_shot.INPUT_TYPES()["required"] == req and list(per_shot.INPUT_TYPES()["optional"]) == ["shots"]
    assert per_shot.propagate is not node.propagate and "shot" in per_shot.DESCRIPTION
    images, masks = torch.zeros(7, 16, 16, 3), torch.zeros(2, 16, 16)
    for cls in (node, per_shot):
        for bad in ("", "6 0", "0 0", "0 7", "-1", "zero"):            # refused before any device is looked for
            with pytest.raises(ValueError):
                cls().propagate(images, masks, bad)
        for bad in ((-1, 16), (8, 16), (2, -1), (2, 256)):
            with pytest.raises(ValueError):
                cls().propagate(images, masks, "0, 6", 4, 2, 8, *bad)
    with pytest.raises(ValueError):                                    # shots that do not end where the clip does
        per_shot().propagate(images, masks, "0, 6", shots=[(0, 3), (3, 6)])
    if not torch.cuda.is_available():
        for cls in (node, per_shot):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                cls().propagate(images, masks, "0, 6", 4, 2, 8, 2, 16)


def test_the_per_shot_form_runs_every_shot_on_its_own_keys(monkeypatch):
    from lanpaint_amd import propagate_keys_anchored_visible as pkav
    from lanpaint_amd import shots
    F, H, W = 10, 4, 5
    images = torch.arange(F, dtype=torch.float32)[:, None, None, None].expand(F, H, W, 3).contiguous()
    calls = []

    def fake(images, masks, keys, *numbers):
        """Frame f of `mask` is the first frame's value + 100 * the number of keys, of `hidden` the first key's mask value."""
        calls.append((images[:, 0, 0, 0].tolist(), masks[:, 0, 0].tolist() if masks.ndim == 3 else masks[0, 0].item(), list(keys), numbers))
        base = images[:, :, :, 0] + 100 * len(keys)
        return base, torch.full_like(base, float(masks.reshape(-1, H, W)[0, 0, 0]))
    monkeypatch.setattr(pkav, "propagate_keys_anchored_visible", fake)
    per_key = torch.tensor([7.0, 8.0, 9.0])[:, None, None].expand(3, H, W).contiguous()
    keys = [1, 2, 8]
    ranges = [(0, 4), (4, 7), (7, 10)]                                 # two keys in the first shot, none in the second, one in the third
    out, hidden = shots.propagate_keys_anchored_visible_shots(images, per_key, ranges, keys, 3, 2, 8, 2, 16)
    assert calls == [([0.0, 1.0, 2.0, 3.0], [7.0, 8.0], [1, 2], (3, 2, 8, 2, 16)), ([7.0, 8.0, 9.0], [9.0], [1], (3, 2, 8, 2, 16))]
    assert out[:, 0, 0].tolist() == [200.0, 201.0, 202.0, 203.0, 0.0, 0.0, 0.0, 107.0, 108.0, 109.0]
    assert hidden[:, 0, 0].tolist() == [7.0] * 4 + [0.0] * 3 + [9.0] * 3
    assert not out[4:7].any() and not hidden[4:7].any() and tuple(out.shape) == tuple(hidden.shape) == (F, H, W)
    del calls[:]
    per_frame = torch.arange(F, dtype=torch.float32)[:, None, None].expand(F, H, W).contiguous() + 50       # [F, H, W]: the keys' are read
    out2, hidden2 = shots.propagate_keys_anchored_visible_shots(images, per_frame, torch.tensor([0] * 4 + [1] * 3 + [2] * 3), keys)
    assert [c[1] for c in calls] == [[51.0, 52.0], [58.0]] and [c[3] for c in calls] == [(4, 2, 8, 2, 16)] * 2     # the defaults
    assert torch.equal(out2, out)
    del calls[:]
    whole = shots.propagate_keys_anchored_visible_shots(images, per_key, [(0, F)], keys, 3, 2, 8, 0, 0)     # a single range: the plain call
    assert calls == [(list(map(float, range(F))), [7.0, 8.0, 9.0], keys, (3, 2, 8, 0, 0))] and whole[0][0, 0, 0] == 300
    for bad_ranges in ([(0, 4), (4, 9)], [(0, 4), (5, 10)], []):
        with pytest.raises(ValueError):
            shots.propagate_keys_anchored_visible_shots(images, per_key, bad_ranges, keys)
    for bad_keys in ([], [2, 1], [0, 10]):
        with pytest.raises(ValueError):
            shots.propagate_keys_anchored_visible_shots(images, per_key, ranges, bad_keys)
    with pytest.raises(ValueError):                                    # two masks for three keys
        shots.propagate_keys_anchored_visible_shots(images, per_key[:2], ranges, keys)
    assert "propagate_keys_anchored_visible_shots" in shots.__doc__


def test_the_new_modules_stay_small():
    names = ("propagate_keys.py", "propagate_keys_visible.py", "propagate_keys_anchored_visible.py",
             "propagate_keys_anchored_visible_nodes.py", "shots.py")
    files = [os.path.join(ROOT, "lanpaint_amd", f) for f in names]
    for f in files:
        assert sum(1 for _ in open(f)) <= 900, f
