"""The anchored video mask propagate from several keyframes, the parts that need no device: the restatement
(tests/propagate_keys_anchored_ref.py) against the single-key anchored one and on the clip the form is for, the warped-key form of
lp_prop_match_batch's argument checks (made before any HIP call), `propagate_keys.Chains` with `rematch` on host memory with its
launches recorded, the wrapper's checks and the node's protocol.  Layouts, constants and names against the header are
tests/test_cabi_mirror.py's, for the whole C ABI.

A descriptor that the library would accept is never handed over here: its addresses are made up, and on a machine with a device
the launch would follow them.  That both forms accept what they should is tests/test_gpu_propagate_keys_anchored.py's, on real
buffers."""
import ctypes
import os

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, _motion, propagate_keys
from tests import propagate_anchored_ref as aref
from tests import propagate_keys_anchored_ref as karef
from tests import propagate_keys_ref as kref
from tests.anchor_clips import iou, subpixel_clip
from tests.compare import _f32_bits as _bits
from tests.device import _match_jobs as _jobs
from tests.propagate_scenes import assert_the_two_gap_iou_lines as assert_the_two_iou_lines, gap_drift_case, lowest_iou

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARPED = _cabi.LP_PROP_MATCH_WARPED_KEY


# ---- the restatement on its own ----------------------------------------------------------------------------------------------------------
def test_the_plain_chains_fall_behind_between_two_keys_and_the_anchored_chains_do_not():
    _, truth, plain, anchored = gap_drift_case()
    assert_the_two_iou_lines(truth, plain, anchored)
    assert round(lowest_iou(plain, truth), 3) == 0.737 and round(lowest_iou(anchored, truth), 3) == 0.871
    assert int(np.argmin([iou(plain[t] >= 0.5, truth[t]) for t in range(49)])) == 23
    for k in (8, 40):                                                  # a key frame returns its binarised painting
        assert (_bits(anchored[k]) == _bits(truth[k].astype(np.float32))).all()


def test_one_key_is_the_single_key_anchored_chain_and_anchor_zero_the_several_keys_rule():
    images, truth = subpixel_clip(7, 23, 33)
    for key in (0, 3, 6):
        mask = truth[key].astype(np.float32)
        for anchor in (1, 2):
            got = karef.propagate_keys_anchored_ref(images, mask[None], [key], 3, 2, 8, anchor)
            assert (_bits(got) == _bits(aref.propagate_anchored_ref(images, mask, key, 3, 2, 8, anchor))).all(), (key, anchor)
    masks = truth[[1, 5]].astype(np.float32)
    assert (_bits(karef.propagate_keys_anchored_ref(images, masks, [1, 5], 3, 2, 8, 0)) ==
            _bits(kref.propagate_keys_ref(images, masks, [1, 5], 3, 2, 8))).all()
    # outside the keys: the single-key anchored chain of that key alone
    got = karef.propagate_keys_anchored_ref(images, masks, [1, 5], 3, 2, 8, 2)
    assert (_bits(got[0]) == _bits(aref.propagate_anchored_ref(images, masks[0], 1, 3, 2, 8, 2)[0])).all()
    assert (_bits(got[6]) == _bits(aref.propagate_anchored_ref(images, masks[1], 5, 3, 2, 8, 2)[6])).all()


def test_still_video_empty_and_full():
    rng = np.random.default_rng(38)
    F, H, W = 6, 23, 33
    video = rng.random((F, H, W, 3), dtype=np.float32)
    still = np.repeat(video[:1], F, axis=0)
    soft = rng.random((H, W), dtype=np.float32)
    binar = (soft >= 0.5).astype(np.float32)
    for keys in ([0, 5], [0, 2, 5]):
        got = karef.propagate_keys_anchored_ref(still, np.repeat(soft[None], len(keys), axis=0), keys, 3, 2, 8, 2)
        assert (_bits(got) == _bits(np.repeat(binar[None], F, axis=0))).all(), keys
        zeros, ones = np.zeros((len(keys), H, W), np.float32), np.ones((len(keys), H, W), np.float32)
        assert (_bits(karef.propagate_keys_anchored_ref(video, zeros, keys, 3, 2, 8, 7)) == 0).all(), keys
        assert (karef.propagate_keys_anchored_ref(video, ones, keys, 3, 2, 8, 7) == 1).all(), keys


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
FIELDS = [f for f, _ in _cabi.LpPropMatchJob._fields_]


def test_the_warped_form_rejects_bad_arguments_without_a_device(hip_lib):
    C, E, J = ctypes, _cabi.LP_E_INVALID, _cabi.LP_PROP_MAX_JOBS
    side = _cabi.LP_VMASK_MAX_SIDE
    a = [256 * (i + 1) for i in range(8)]                             # never dereferenced: every descriptor here is refused
    good_job = (a[0], a[1], a[2], a[3], a[4], a[5])
    keep, ptr = _jobs([good_job] * J)
    good = dict(height=40, width=70, levels=3, level=0, search=2, smooth=8, jobs=2, reserved0=WARPED, job=ptr)

    def call(**change):
        return hip_lib.lp_prop_match_batch(C.byref(_cabi.LpPropMatchBatchDesc(**{**good, **change})), None)
    for change in ({"level": 1}, {"level": 2}, {"level": -1}, {"levels": 1, "level": 1}, {"search": 0}, {"search": 8}, {"search": -1},
                   {"smooth": -1}, {"smooth": 65}, {"height": 0}, {"width": side + 1}, {"levels": 0}, {"levels": 7}, {"jobs": 0},
                   {"jobs": J + 1}, {"job": None}):
        assert call(**change) == E, change
    for value in (2, -1, 3, 1 << 16, -(1 << 31)):                      # no other source form exists, whatever else is right
        assert call(reserved0=value) == E, value
        assert call(reserved0=value, level=1) == E, value              # nor next to what form 0 would take
    for at in (0, 1, J - 1):                                          # one bad job anywhere in the table
        bad = [(f, None) for f in FIELDS]                              # a null pointer, the positions in `parent` included
        bad += [(out, a[FIELDS.index(inp)]) for out in ("vec", "valid") for inp in ("src", "tgt", "mask", "parent")]
        bad += [("vec", a[5]), ("valid", a[4])]                        # the two outputs on one another
        for levels in (1, 3):                                          # a null parent is refused at levels 1 too: it is P_t
            for field, value in bad:
                rows = [list(good_job) for _ in range(J)]
                rows[at][FIELDS.index(field)] = value
                keep2, ptr2 = _jobs(rows)
                assert call(levels=levels, jobs=at + 1, job=ptr2) == E, (at, levels, field, value)


def test_form_zero_refuses_what_it_refused(hip_lib):
    """reserved0 = 0, spelled out: the list of tests/test_propagate_keys_host.py, and where the two forms part -- form 0 wants no
    parent at the top level, the warped form wants its positions there."""
    C, E, J = ctypes, _cabi.LP_E_INVALID, _cabi.LP_PROP_MAX_JOBS
    a = [256 * (i + 1) for i in range(8)]
    good_job = (a[0], a[1], a[2], a[3], a[4], a[5])
    keep, ptr = _jobs([good_job] * J)
    good = dict(height=40, width=70, levels=3, level=1, search=2, smooth=8, jobs=2, reserved0=0, job=ptr)

    def call(**change):
        return hip_lib.lp_prop_match_batch(C.byref(_cabi.LpPropMatchBatchDesc(**{**good, **change})), None)
    for change in ({"height": 0}, {"levels": 0}, {"levels": 7}, {"level": -1}, {"level": 3}, {"search": 0}, {"search": 8},
                   {"smooth": -1}, {"smooth": 65}, {"jobs": 0}, {"jobs": J + 1}, {"job": None},
                   {"level": 2}, {"levels": 1, "level": 0}):           # the top level with parents given
        assert call(**change) == E, change
    for field, value in (("src", None), ("tgt", None), ("mask", None), ("vec", None), ("valid", None), ("parent", None), ("parent", a[4])):
        rows = [list(good_job) for _ in range(2)]
        rows[1][FIELDS.index(field)] = value
        keep2, ptr2 = _jobs(rows)
        assert call(job=ptr2) == E, field
    assert ctypes.sizeof(_cabi.LpPropMatchBatchDesc) == 40 and _cabi.LpPropMatchBatchDesc.reserved0.offset == 28


def test_no_new_entry_and_the_words_are_everywhere():
    assert not [name for name in _cabi.EXPORTS if "keys_anchored" in name or "warped" in name]      # no new entry
    header = open(os.path.join(ROOT, "include", "lanpaint_hip.h")).read()
    for word in ("Video mask propagate from several keys, anchored", "LP_PROP_MATCH_WARPED_KEY", "is the anchored chain of its key",
                 "the merge are unchanged", "required whatever `levels` is", "Not handled: occlusion.",
                 "re-anchoring every n-th frame only"):
        assert word in header, word
    assert "re-anchoring against drift" not in header
    for doc in ("README.md", "DESIGN.md", "CHANGES.md", "INTEGRATION.md"):
        assert "LanPaint_VideoMaskPropagateKeysAnchored" in open(os.path.join(ROOT, doc)).read(), doc
    from lanpaint_amd import propagate_anchored
    assert "propagate_keys_anchored.py" in propagate_anchored.__doc__ and "propagate_keys_visible.py" in propagate_anchored.__doc__


# ---- the chain table with the option on ---------------------------------------------------------------------------------------------------
def test_the_chains_tables_with_rematch(monkeypatch):
    """`propagate_keys.Chains(..., rematch=(2,))` on host memory, its launches recorded: 6 frames with keys on 1 and 4, so an edge
    chain backwards of 1 step, the gap's forward and backward chains of 2 steps and an edge chain forwards of 1 step.  For steps 1
    and 2: the entries in order, each descriptor's numbers, `jobs` and source form, and every row of every table against addresses
    worked out by hand from the buffers' `data_ptr()` and row sizes."""
    H, W, levels, search, smooth, anchor, F = 20, 12, 2, 3, 5, 2, 6
    plan = propagate_keys.chain_plan(F, [1, 4])
    assert plan == [(0, 1, -1, 1), (0, 1, 1, 2), (1, 4, -1, 2), (1, 4, 1, 1)]
    stride = _cabi.prop_pyramid_ws_bytes(1, H, W, levels)
    plane, positions = H * W * 4, H * W * 2 * 4                        # fp32 [H, W], int32 [H, W, 2]: bytes a row
    pyr = torch.zeros((F, stride), dtype=torch.uint8)
    key_pyrs = [torch.zeros((1, stride), dtype=torch.uint8) for _ in range(2)]
    out, back = torch.zeros((F, H, W), dtype=torch.float32), torch.zeros((2, H, W), dtype=torch.float32)
    at = lambda t: t.data_ptr()                                        # noqa: E731
    outs = [(at(out) + plane, -plane), (at(out) + plane, plane), (at(back) + 2 * plane, -plane), (at(out) + 4 * plane, plane)]
    columns = {"lp_prop_match_batch": 6, "lp_prop_fill_batch": 3, "lp_prop_advance_batch": 6}
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
    with pytest.raises(ValueError, match="rematch with split"):
        propagate_keys.Chains(plan, pyr, key_pyrs, outs, H, W, levels, search, smooth, split=(16, outs, outs, outs, outs), rematch=(anchor,))
    for bad in ((0,), (8,), (2.0,), (True,)):
        with pytest.raises(ValueError):
            propagate_keys.Chains(plan, pyr, key_pyrs, outs, H, W, levels, search, smooth, rematch=bad)
    chains = propagate_keys.Chains(plan, pyr, key_pyrs, outs, H, W, levels, search, smooth, rematch=(anchor,))

    i32, u8 = torch.int32, torch.uint8
    assert [(tuple(t.shape), t.dtype) for t in chains._keep] == [((4, H, W, 2), i32)] * 2 + [((4, stride), u8)] * 2 + \
        [((4, H, W, 2), i32), ((4, stride), u8)]
    pos, mpyr, raw_pos, raw_mpyr = chains._keep[0:2], chains._keep[2:4], chains._keep[4], chains._keep[5]
    raw0, valid0, field0, raw1, valid1, field1 = chains.walk._keep
    assert [tuple(t.shape) for t in chains.walk._keep] == [(4, 3, 2, 2), (4, 3, 2), (4, 3, 2, 2), (4, 2, 1, 2), (4, 2, 1), (4, 2, 1, 2)]

    def want_step(s, active):
        """The launches of step s for the chains `active` of the plan: chain c is row j of every table."""
        rows = {name: [] for name in ("match1", "fill1", "match0", "fill0", "first", "rematch", "second")}
        for j, c in enumerate(active):
            i, k, d, _ = plan[c]
            src, tgt = at(pyr) + (k + d * (s - 1)) * stride, at(pyr) + (k + d * s) * stride
            weight = at(key_pyrs[i]) if s == 1 else at(mpyr[(s - 1) & 1]) + c * stride
            pos_src = 0 if s == 1 else at(pos[(s - 1) & 1]) + c * positions
            pos_t, mpyr_t = at(pos[s & 1]) + c * positions, at(mpyr[s & 1]) + c * stride
            raw_pos_t, bits = at(raw_pos) + c * positions, at(raw_mpyr) + c * stride       # the chain's, not the group's
            r1, v1, f1 = at(raw1) + j * 16, at(valid1) + j * 8, at(field1) + j * 16      # the walk's rows are the group's
            r0, v0, f0 = at(raw0) + j * 48, at(valid0) + j * 24, at(field0) + j * 48
            written = outs[c][0] + s * outs[c][1]
            rows["match1"].append([src, tgt, weight, 0, r1, v1])
            rows["fill1"].append([r1, v1, f1])
            rows["match0"].append([src, tgt, weight, f1, r0, v0])
            rows["fill0"].append([r0, v0, f0])
            rows["first"].append([f0, pos_src, at(key_pyrs[i]), raw_pos_t, written, bits])
            rows["rematch"].append([at(pyr) + k * stride, tgt, bits, raw_pos_t, r0, v0])   # the key frame's luma, the frame's
            rows["second"].append([f0, raw_pos_t, at(key_pyrs[i]), pos_t, written, mpyr_t])
        return [("lp_prop_match_batch", [H, W, levels, 1, search, smooth, 0], rows["match1"]), ("lp_prop_fill_batch", [2, 1], rows["fill1"]),
                ("lp_prop_match_batch", [H, W, levels, 0, search, smooth, 0], rows["match0"]), ("lp_prop_fill_batch", [3, 2], rows["fill0"]),
                ("lp_prop_advance_batch", [H, W, levels], rows["first"]),
                ("lp_prop_match_batch", [H, W, levels, 0, anchor, smooth, WARPED], rows["rematch"]),
                ("lp_prop_fill_batch", [3, 2], rows["fill0"]),
                ("lp_prop_advance_batch", [H, W, levels], rows["second"])]

    chains.step(1)
    assert len(launched) == 2 * levels + 4
    assert launched == want_step(1, [0, 1, 2, 3])
    assert all(row[1] == 0 for row in launched[4][2])                  # a null pos_src: the key frame's positions
    assert [row[1] for row in launched[7][2]] == [at(raw_pos) + c * positions for c in range(4)]   # the second advance reads P_t
    assert [row[0] for row in launched[5][2]] == [at(pyr) + k * stride for k in (1, 1, 4, 4)]      # each chain's own key frame
    del launched[:]
    chains.step(2)
    assert launched == want_step(2, [1, 2]) and all(len(rows) == 2 for _, _, rows in launched)
    assert [row[1] for row in launched[4][2]] == [at(pos[1]) + c * positions for c in (1, 2)]       # read what step 1's second
    assert [row[3] for row in launched[7][2]] == [at(pos[0]) + c * positions for c in (1, 2)]       # advance wrote, write the other
    assert [row[2] for row in launched[0][2]] == [at(mpyr[1]) + c * stride for c in (1, 2)]         # the second advance's bits weigh
    assert [row[4] for row in launched[7][2]] == [at(out[3]), at(back[0])]                          # frame 3, and frame 2 in the stack
    del launched[:]
    chains.step(3)
    assert launched == []


def test_rematch_off_allocates_and_launches_what_it_did(monkeypatch):
    H, W, levels, F = 20, 12, 2, 6
    plan = propagate_keys.chain_plan(F, [1, 4])
    stride = _cabi.prop_pyramid_ws_bytes(1, H, W, levels)
    pyr, key_pyrs = torch.zeros((F, stride), dtype=torch.uint8), [torch.zeros((1, stride), dtype=torch.uint8) for _ in range(2)]
    out = torch.zeros((F, H, W), dtype=torch.float32)
    outs = [(out.data_ptr(), 0)] * 4
    names = []
    for module in (_motion, propagate_keys):
        monkeypatch.setattr(module, "launch", lambda entry, *a: names.append(entry))
    for off in ({}, {"rematch": None}, {"rematch": ()}):
        chains = propagate_keys.Chains(plan, pyr, key_pyrs, outs, H, W, levels, 3, 5, **off)
        assert len(chains._keep) == 4 and not hasattr(chains, "raw_pos") and not hasattr(chains, "t_rematch")
        del names[:]
        chains.step(1)
        assert names == ["lp_prop_match_batch", "lp_prop_fill_batch"] * levels + ["lp_prop_advance_batch"]


# ---- the wrappers and the node ----------------------------------------------------------------------------------------------------------
def test_propagate_keys_anchored_refuses_cpu_tensors_and_bad_arguments():
    from lanpaint_amd import propagate_keys_anchored as pka
    images, masks = torch.zeros(7, 16, 16, 3), torch.zeros(2, 16, 16)
    for anchor in (0, 2):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pka.propagate_keys_anchored(images, masks, [0, 6], anchor=anchor)
    row = torch.zeros(_cabi.prop_pyramid_ws_bytes(1, 16, 16, 3), dtype=torch.uint8)
    positions = torch.zeros(16, 16, 2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pka.anchor_field_batch([(row, row, row, positions)], 16, 16, 3, 2, 8)
    assert pka.anchor_field_batch is propagate_keys.anchor_field_batch
    # the numbers are checked before the tensors are looked at
    for bad in (dict(levels=0), dict(levels=7), dict(search=0), dict(search=8), dict(smooth=-1), dict(smooth=65), dict(anchor=-1),
                dict(anchor=8), dict(anchor=2.0), dict(anchor=True), dict(anchor=None)):
        with pytest.raises(ValueError):
            pka.propagate_keys_anchored(images, masks, [0, 6], **bad)
    for bad in (dict(anchor=0), dict(anchor=8), dict(smooth=65), dict(levels=0)):
        with pytest.raises(ValueError):
            pka.anchor_field_batch([(row, row, row, positions)], 16, 16, **{"levels": 3, "anchor": 2, "smooth": 8, **bad})
    for keys in ([], [6, 0], [0, 0], [0, 7], [-1, 3], [0.0, 6], None, 3):
        for anchor in (0, 2):
            with pytest.raises(ValueError):
                pka.propagate_keys_anchored(images, masks, keys, anchor=anchor)
    assert pka.DEFAULT_ANCHOR == 2 and pka.MAX_ANCHOR == 7


def test_keys_anchored_node_protocol_and_own_mappings():
    from lanpaint_amd import propagate_keys_anchored_nodes, propagate_keys_nodes, propagate_nodes
    node = propagate_keys_anchored_nodes.LanPaint_VideoMaskPropagateKeysAnchored
    assert propagate_keys_anchored_nodes.NODE_CLASS_MAPPINGS == {"LanPaint_VideoMaskPropagateKeysAnchored": node}
    assert propagate_keys_anchored_nodes.NODE_DISPLAY_NAME_MAPPINGS == {
        "LanPaint_VideoMaskPropagateKeysAnchored": "LanPaint Video Mask Propagate (Keys, Anchored)"}
    assert propagate_keys_nodes.NODE_CLASS_MAPPINGS == {"LanPaint_VideoMaskPropagateKeys": propagate_keys_nodes.LanPaint_VideoMaskPropagateKeys}
    assert propagate_keys_anchored_nodes.parse_key_frames is propagate_keys_nodes.parse_key_frames
    types = node.INPUT_TYPES()
    req = types["required"]
    assert list(types) == ["required"] and list(req) == ["image", "mask", "key_frames", "levels", "search", "smooth", "anchor"]
    keys_req = propagate_keys_nodes.LanPaint_VideoMaskPropagateKeys.INPUT_TYPES()["required"]
    for name in ("levels", "search", "smooth"):
        assert req[name] == keys_req[name] == propagate_nodes.MATCHER_WIDGETS[name], name
    assert req["image"][0] == "IMAGE" and req["mask"][0] == "MASK"
    assert req["key_frames"][0] == "STRING" and req["key_frames"][1]["default"] == "0"
    assert req["anchor"][0] == "INT" and req["anchor"][1] == {**req["anchor"][1], "default": 2, "min": 0, "max": 7}
    for name in req:
        assert len(req[name][1]["tooltip"]) > 20, name
    assert node.RETURN_TYPES == ("MASK",) and node.RETURN_NAMES == ("mask",)
    assert node.FUNCTION == "propagate" and node.CATEGORY == "mask" and callable(getattr(node, node.FUNCTION))
    for word in ("key frames", "motion", "merged", "key frame again", "long gap", "stabilize", "mask refine", "encode", "Detailer",
                 "Occlusion", "empty key", "drifts as before"):
        assert word in node.DESCRIPTION, word
    images, masks = torch.zeros(7, 16, 16, 3), torch.zeros(2, 16, 16)
    for bad in ("", "6 0", "0 0", "0 7", "-1", "zero"):               # refused before any device is looked for
        with pytest.raises(ValueError):
            node().propagate(images, masks, bad)
    for bad in (-1, 8):
        with pytest.raises(ValueError):
            node().propagate(images, masks, "0, 6", 4, 2, 8, bad)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            node().propagate(images, masks, "0, 6", 4, 2, 8, 2)


def test_the_new_modules_stay_small():
    names = ("propagate_keys.py", "propagate_keys_anchored.py", "propagate_keys_anchored_nodes.py")
    files = [os.path.join(ROOT, "lanpaint_amd", f) for f in names]
    for f in files:
        assert sum(1 for _ in open(f)) <= 900, f
