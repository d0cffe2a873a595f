"""The motion modules' shared host layer (lanpaint_amd/_motion.py, and `tensor_is` in _hostcall.py) where no device is needed: the
checks' messages, and the job tables of the field walk against addresses worked out by hand.  The device rule is switched off
for the checks behind it; the walk runs on host memory with its launches recorded instead of made."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, _hostcall, _motion, propagate_keys, propagate_keys_visible

MODULE = "lanpaint_amd.some_module"


def test_tensor_is_refuses_a_tensor_off_the_device_first():
    for bad in (torch.zeros(2, 3), np.zeros((2, 3), np.float32), None):
        with pytest.raises(RuntimeError, match=r"lanpaint_amd\.some_module runs on a HIP device only; no CPU fallback \(flags is not"):
            _hostcall.tensor_is(bad, torch.float32, (2, 3), "flags", MODULE)
    with pytest.raises(RuntimeError, match=r"some_module.*no CPU fallback \(mask is not"):
        _motion.clip_mask(torch.zeros(4, 5), 3, 4, 5, MODULE)


def test_tensor_is_names_the_argument_the_expectation_and_what_was_given(monkeypatch):
    monkeypatch.setattr(_hostcall, "require_hip", lambda t, what, module: t)
    good = torch.zeros((3, 4, 2), dtype=torch.int32)
    assert _hostcall.tensor_is(good, torch.int32, (3, 4, 2), "vec", MODULE) is good
    assert _hostcall.tensor_is(good, torch.int32, (None, 4, 2), "vec", MODULE) is good
    assert _hostcall.tensor_is(good, torch.int32, good.shape, "vec", MODULE) is good
    assert _hostcall.tensor_is(good[:0], torch.int32, (None, 4, 2), "vec", MODULE).shape[0] == 0
    wrong = {"dtype": (good.float(), (3, 4, 2)), "a size": (good, (3, 5, 2)), "a size behind a free one": (good, (None, 4, 3)),
             "fewer dimensions": (good[0], (3, 4, 2)), "more dimensions": (good[None], (3, 4, 2)),
             "not contiguous": (good.transpose(0, 1), (4, 3, 2)), "a strided row": (good[:, :, :1], (3, 4, 1))}
    for what, (t, shape) in wrong.items():
        with pytest.raises(ValueError) as e:
            _hostcall.tensor_is(t, torch.int32, shape, "vec", MODULE)
        want = ", ".join("n" if n is None else str(n) for n in shape)
        assert str(e.value) == f"vec must be a contiguous torch.int32 [{want}], got {t.dtype} {list(t.shape)}", what


def test_clip_mask_takes_three_shapes_and_names_what_it_refuses(monkeypatch):
    monkeypatch.setattr(_motion, "require_hip", lambda t, what, module: t)
    F, H, W = 3, 4, 5
    one = torch.zeros(H, W)
    assert _motion.clip_mask(one, F, H, W, MODULE).shape == (1, H, W)
    assert _motion.clip_mask(one[None], F, H, W, MODULE).shape == (1, H, W)
    assert _motion.clip_mask(torch.zeros(F, H, W), F, H, W, MODULE).shape == (F, H, W)
    for bad in (torch.zeros(2, H, W), torch.zeros(F, H, W + 1), torch.zeros(H + 1, W), torch.zeros(1, 1, H, W), torch.zeros(W)):
        with pytest.raises(ValueError) as e:
            _motion.clip_mask(bad, F, H, W, MODULE)
        given = (1, *bad.shape) if bad.ndim == 2 else tuple(bad.shape)      # a plane is named as the [1, H, W] it was taken for
        assert str(e.value) == f"mask {given} does not match 3 frames of 4x5: [H, W], [1, H, W] or [F, H, W]"


def test_the_numbers_and_the_plane(monkeypatch):
    for bad in ((0, 2, 8), (_motion.MAX_LEVELS + 1, 2, 8), (3, 0, 8), (3, _motion.MAX_SEARCH + 1, 8), (3, 2, -1), (3, 2, _motion.MAX_SMOOTH + 1),
                (3.0, 2, 8), (3, True, 8)):
        with pytest.raises(ValueError, match="levels|search|smooth"):
            _motion.check_params(*bad)
    _motion.check_params(_motion.MAX_LEVELS, _motion.MAX_SEARCH, _motion.MAX_SMOOTH)
    for bad in ((0, 5), (5, 0), (_motion.MAX_SIDE + 1, 5)):
        with pytest.raises(ValueError, match="plane: sides 1.."):
            _motion.check_plane(*bad)
    with pytest.raises(RuntimeError, match=r"no CPU fallback \(images is not"):
        _motion.check_images(torch.zeros(2, 4, 5, 3))
    monkeypatch.setattr(_motion, "require_hip", lambda t, what, module: t)
    for bad in (torch.zeros(4, 5, 3), torch.zeros(2, 4, 5, _cabi.LP_DETAIL_MAX_CHANNELS + 1), torch.zeros(2, 0, 5, 3)):
        with pytest.raises(ValueError, match=r"images must be \[F, H, W, C\]"):
            _motion.check_images(bad)
    pyr = torch.arange(2 * _cabi.prop_pyramid_ws_bytes(1, 9, 7, 2), dtype=torch.uint8).view(2, -1)
    top = _motion.level_view(pyr, 9, 7, 1)
    off = _cabi.prop_level_offset(9, 7, 1)
    assert off >= 63 and top.shape == (2, 5, 4) and top[1, 0, 0] == pyr[1, off] and top.data_ptr() == pyr.data_ptr() + off


def test_the_walks_tables_for_two_jobs_and_two_levels(monkeypatch):
    """What `temporal_fill.step_fields` and `propagate_keys.Chains` have the walk write into its tables, as each wrote them itself
    before the walk was shared: per level a match row (source, target, weights, the level above's field or 0, raw, valid) and a fill row (raw, valid, field), the
    top level launched first, level 0's field at the caller's address or in the walk's own row."""
    H, W, levels, search, smooth = 20, 12, 2, 3, 5
    grids = [_cabi.prop_grid(H, W, lv) for lv in range(levels)]
    assert grids == [(3, 2), (2, 1)]
    launched = []

    def record(entry, dev, *args):
        lv = (len(launched) // 2 + 1) % 2                              # two launches a level, level 1 first
        if entry == "lp_prop_match_batch":
            d = walk.desc[lv]
            assert ctypes.addressof(args[0]._obj) == ctypes.addressof(d) and d.job == walk.t_match[lv].ctypes.data
            assert (d.height, d.width, d.levels, d.level, d.search, d.smooth) == (H, W, levels, lv, search, smooth)
            launched.append((entry, d.jobs, walk.t_match[lv][:d.jobs].copy()))
        else:
            table, jobs, gh, gw = args
            assert table == walk.t_fill[lv].ctypes.data and (gh, gw) == grids[lv]
            launched.append((entry, jobs, walk.t_fill[lv][:jobs].copy()))
    monkeypatch.setattr(_motion, "launch", record)
    for m, level0 in ((2, True), (3, False)):
        walk = _motion.FieldWalk(m, H, W, levels, search, smooth, torch.device("cpu"), level0=level0)
        kept = iter(walk._keep)
        raw0, valid0, field0 = next(kept), next(kept), (next(kept) if level0 else None)
        raw1, valid1, field1 = next(kept), next(kept), next(kept)
        assert [tuple(t.shape) for t in (raw0, valid0, raw1, valid1, field1)] == [(m, 3, 2, 2), (m, 3, 2), (m, 2, 1, 2), (m, 2, 1), (m, 2, 1, 2)]
        assert all(t.dtype == torch.int32 for t in walk._keep) and len(walk._keep) == 5 + level0

        def rows(t, row_bytes):                                        # by hand: 4 bytes an int32, rows back to back
            return [t.data_ptr(), t.data_ptr() + row_bytes]
        src, tgt, weight, out = [1000, 2000], [3000, 4000], [5000, 6000], [7000, 7048]
        want_field0 = rows(field0, 48) if level0 else out
        want = [("lp_prop_match_batch", [src, tgt, weight, [0, 0], rows(raw1, 16), rows(valid1, 8)]),
                ("lp_prop_fill_batch", [rows(raw1, 16), rows(valid1, 8), rows(field1, 16)]),
                ("lp_prop_match_batch", [src, tgt, weight, rows(field1, 16), rows(raw0, 48), rows(valid0, 24)]),
                ("lp_prop_fill_batch", [rows(raw0, 48), rows(valid0, 24), want_field0])]
        del launched[:]
        u64 = lambda a: np.array(a, dtype=np.uint64)                   # noqa: E731
        walk.run(u64(src), u64(tgt), u64(weight), None if level0 else u64(out))
        assert [(e, n) for e, n, _ in launched] == [(e, 2) for e, _ in want]
        for (entry, _, table), (_, columns) in zip(launched, want):
            assert table.dtype == np.uint64 and table.tolist() == [list(r) for r in zip(*columns)], entry
        if level0:
            assert walk.field0.tolist() == want_field0
            walk.run(u64(src), u64(tgt), u64(weight), u64(out))        # told once where level 0 goes, then not: back in its own rows
            walk.run(u64(src[:1]), u64(tgt[:1]), u64(weight[:1]))
            assert launched[-1][1] == 1 and launched[-1][2].tolist() == [[raw0.data_ptr(), valid0.data_ptr(), field0.data_ptr()]]
    with pytest.raises(ValueError):
        _motion.FieldWalk(_motion.MAX_JOBS + 1, H, W, levels, search, smooth, torch.device("cpu"))


@pytest.mark.parametrize("option", [False, True], ids=["plain", "occlusion-aware"])
def test_the_chains_tables_for_all_three_chain_cases(option, monkeypatch):
    """`propagate_keys.Chains` on host memory, its launches recorded: 6 frames with keys on 1 and 4, so an edge chain backwards of 1
    step, the gap's forward and backward chains of 2 steps and an edge chain forwards of 1 step.  For the count of the keys' bits and
    for steps 1 and 2: the entries in order, each descriptor's numbers and `jobs`, and every row of every table against addresses
    worked out by hand from the buffers' `data_ptr()` and row sizes -- with the occlusion-aware option off and on."""
    H, W, levels, search, smooth, occlusion, F = 20, 12, 2, 3, 5, 16, 6
    plan = propagate_keys.chain_plan(F, [1, 4])
    assert plan == [(0, 1, -1, 1), (0, 1, 1, 2), (1, 4, -1, 2), (1, 4, 1, 1)]
    stride = _cabi.prop_pyramid_ws_bytes(1, H, W, levels)
    plane, cells, positions = H * W * 4, 3 * 2 * 4, H * W * 2 * 4      # fp32 [H, W], int32 [3, 2], int32 [H, W, 2]: bytes a row
    f32, i32 = torch.float32, torch.int32
    pyr = torch.zeros((F, stride), dtype=torch.uint8)
    key_pyrs = [torch.zeros((1, stride), dtype=torch.uint8) for _ in range(2)]
    out, hidden, scratch = torch.zeros((F, H, W), dtype=f32), torch.zeros((F, H, W), dtype=f32), torch.zeros((4, H, W), dtype=f32)
    at = lambda t: t.data_ptr()                                        # noqa: E731
    if option:                  # per chain (address, byte step): step s is at address + s * step
        back, flags = torch.zeros((2, 2, H, W), dtype=f32), torch.zeros((2, 2, 3, 2), dtype=i32)
        scratch_flags, counts = torch.zeros((5, 3, 2), dtype=i32), torch.zeros(6, dtype=i32)
        # the edge chains: the code in a fixed scratch row, mask and hidden in the outputs, the flags in a fixed row, no count
        # the gap's forward chain, frame 1 + s: code and mask in place in `hidden` and `out`, its flags at row s - 1 of a stack
        # the gap's backward chain, frame 4 - s: row 2 - s of its stacks
        code = [(at(scratch[0]), 0), (at(hidden) + plane, plane), (at(back[0]) + 2 * plane, -plane), (at(scratch[3]), 0)]
        mask = [(at(out) + plane, -plane), (at(out) + plane, plane), (at(back[1]) + 2 * plane, -plane), (at(out) + 4 * plane, plane)]
        hid = [(at(hidden) + plane, -plane), (at(scratch[1]), 0), (at(scratch[2]), 0), (at(hidden) + 4 * plane, plane)]
        flag = [(at(scratch_flags[0]), 0), (at(flags[0]) - cells, cells), (at(flags[1]) + 2 * cells, -cells), (at(scratch_flags[3]), 0)]
        count = [(0, 0), (at(counts), 4), (at(counts) + 3 * 4, 4), (0, 0)]
        outs, split = code, (occlusion, mask, hid, flag, count)
        assert at(flags[1]) == at(flags) + 2 * cells and at(back[1]) == at(back) + 2 * plane and at(scratch[3]) == at(scratch) + 3 * plane
    else:
        back = torch.zeros((2, H, W), dtype=f32)
        outs, split = [(at(out) + plane, -plane), (at(out) + plane, plane), (at(back) + 2 * plane, -plane), (at(out) + 4 * plane, plane)], None
    # where the case says: frames 0, 2 and 3, rows 1 and 0 of the backward stack, frame 5
    assert [[b + s * step for s in range(1, n + 1)] for (b, step), (_, _, _, n) in zip(outs if not option else split[1], plan)] == [
        [at(out[0])], [at(out[2]), at(out[3])], [at(back[1][1] if option else back[1]), at(back[1][0] if option else back[0])], [at(out[5])]]

    columns = {"lp_prop_match_batch": 6, "lp_prop_fill_batch": 3, "lp_prop_advance_batch": 6, "lp_prop_visible_batch": 5,
               "lp_prop_occlude_batch": 6}
    launched = []

    def record(entry, dev, *args):
        if entry == "lp_prop_fill_batch":
            table, jobs, *numbers = args
        else:
            d = args[0]._obj
            table, jobs = d.job, d.jobs
            numbers = [getattr(d, name) for name, _ in d._fields_ if name not in ("jobs", "job", "reserved0")]
        rows = np.ctypeslib.as_array((ctypes.c_uint64 * (jobs * columns[entry])).from_address(table)).reshape(jobs, columns[entry])
        launched.append((entry, numbers, rows.tolist()))
    for module in (_motion, propagate_keys, propagate_keys_visible):
        monkeypatch.setattr(module, "launch", record)
    chains = propagate_keys.Chains(plan, pyr, key_pyrs, outs, H, W, levels, search, smooth, split=split)

    pos, mpyr = chains._keep[0:2], chains._keep[2:4]
    assert [tuple(t.shape) for t in chains._keep[:4]] == [(4, H, W, 2)] * 2 + [(4, stride)] * 2 and len(chains._keep) == 4 + option
    assert [t.dtype for t in chains._keep[:4]] == [i32, i32, torch.uint8, torch.uint8]
    if option:
        raw_mpyr = chains._keep[4]
        assert tuple(raw_mpyr.shape) == (4, stride) and raw_mpyr.dtype == torch.uint8
    raw0, valid0, field0, raw1, valid1, field1 = chains.walk._keep
    assert [tuple(t.shape) for t in chains.walk._keep] == [(4, 3, 2, 2), (4, 3, 2), (4, 3, 2, 2), (4, 2, 1, 2), (4, 2, 1), (4, 2, 1, 2)]

    def want_step(s, active):
        """The launches of step s for the chains `active` of the plan: chain c is row j of every table."""
        rows = {name: [] for name in ("match1", "fill1", "match0", "fill0", "advance", "visible", "occlude")}
        for j, c in enumerate(active):
            i, k, d, _ = plan[c]
            src, tgt = at(pyr) + (k + d * (s - 1)) * stride, at(pyr) + (k + d * s) * stride
            weight = at(key_pyrs[i]) if s == 1 else at(mpyr[(s - 1) & 1]) + c * stride
            pos_src = 0 if s == 1 else at(pos[(s - 1) & 1]) + c * positions
            pos_t, mpyr_t = at(pos[s & 1]) + c * positions, at(mpyr[s & 1]) + c * stride
            r1, v1, f1 = at(raw1) + j * 16, at(valid1) + j * 8, at(field1) + j * 16      # the walk's rows are the group's, not the chain's
            r0, v0, f0 = at(raw0) + j * 48, at(valid0) + j * 24, at(field0) + j * 48
            rows["match1"].append([src, tgt, weight, 0, r1, v1])
            rows["fill1"].append([r1, v1, f1])
            rows["match0"].append([src, tgt, weight, f1, r0, v0])
            rows["fill0"].append([r0, v0, f0])
            written = outs[c][0] + s * outs[c][1]                      # the mask, or with the option the code
            if option:
                bits = at(raw_mpyr) + c * stride
                mask_t, hidden_t, flags_t, count_t = (col[c][0] + s * col[c][1] for col in split[1:])
                rows["advance"].append([f0, pos_src, at(key_pyrs[i]), pos_t, written, bits])
                rows["visible"].append([pos_t, tgt, at(pyr) + k * stride, bits, flags_t])
                rows["occlude"].append([written, flags_t, mask_t, hidden_t, mpyr_t, count_t])
            else:
                rows["advance"].append([f0, pos_src, at(key_pyrs[i]), pos_t, written, mpyr_t])
        want = [("lp_prop_match_batch", [H, W, levels, 1, search, smooth], rows["match1"]), ("lp_prop_fill_batch", [2, 1], rows["fill1"]),
                ("lp_prop_match_batch", [H, W, levels, 0, search, smooth], rows["match0"]), ("lp_prop_fill_batch", [3, 2], rows["fill0"]),
                ("lp_prop_advance_batch", [H, W, levels], rows["advance"])]
        if option:
            want += [("lp_prop_visible_batch", [H, W, occlusion], rows["visible"]), ("lp_prop_occlude_batch", [H, W, levels], rows["occlude"])]
        return want

    if option:                                                         # the keys' bits of the gap's two chains, before step 1
        painted, zero_flags = [out[k] for _, k, _, _ in plan], scratch_flags[4]
        chains.count_keys(painted, zero_flags)
        assert launched == [("lp_prop_occlude_batch", [H, W, levels], [
            [at(painted[c]), at(zero_flags), at(pos[0]) + c * positions, at(scratch[c]), at(mpyr[0]) + c * stride, count[c][0]] for c in (1, 2)])]
        del launched[:]
    chains.step(1)
    assert launched == want_step(1, [0, 1, 2, 3])
    assert all(row[1] == 0 for row in launched[4][2])                  # a null pos_src: the key frame's positions
    assert [row[2] for row in launched[0][2]] == [at(key_pyrs[0]), at(key_pyrs[0]), at(key_pyrs[1]), at(key_pyrs[1])]   # the key's pyramid weighs
    del launched[:]
    chains.step(2)
    want = want_step(2, [1, 2])                                        # the two surviving chains in rows 0 and 1
    assert launched == want and all(len(rows) == 2 for _, _, rows in launched)
    assert [row[1] for row in launched[4][2]] == [at(pos[1]) + c * positions for c in (1, 2)]       # read what step 1 wrote,
    assert [row[3] for row in launched[4][2]] == [at(pos[0]) + c * positions for c in (1, 2)]       # write the other of the pair
    assert [row[2] for row in launched[0][2]] == [at(mpyr[1]) + c * stride for c in (1, 2)]
    del launched[:]
    chains.step(3)
    assert launched == []


def test_the_gap_layout_and_the_three_chain_cases_by_hand():
    """`propagate_keys.Gaps` for keys 1, 4, 5, 9 in 11 frames: two gaps (4 and 5 are neighbours), the second one's rows behind the
    first one's in a stack of all five in-between frames; and where step s of every chain goes, (address, byte step) by hand."""
    keys = [1, 4, 5, 9]
    plan = propagate_keys.chain_plan(11, keys)
    assert plan == [(0, 1, -1, 1), (0, 1, 1, 2), (1, 4, -1, 2), (2, 5, 1, 3), (3, 9, -1, 3), (3, 9, 1, 1)]
    gaps = propagate_keys.Gaps(keys)
    assert gaps.pairs == [(1, 4), (5, 9)] and gaps.first == {(1, 4): 0, (5, 9): 2} and gaps.between == 5
    assert [gaps.of(c) for c in plan] == [None, (1, 4), (1, 4), (5, 9), (5, 9), None]
    out, stack = torch.zeros((11, 3, 5)), torch.zeros((2, 5, 2, 3), dtype=torch.int32)[1]      # rows of 60 and of 24 bytes
    o, t = out.data_ptr(), stack.data_ptr()
    assert [gaps.in_place(out, c) for c in plan] == [(o + 60, -60), (o + 60, 60), (o + 4 * 60, -60), (o + 5 * 60, 60), (o + 9 * 60, -60),
                                                     (o + 9 * 60, 60)]
    # forwards, frame a + s is row first + s - 1; backwards, frame b - s is row first + length - s
    assert [gaps.stacked(stack, c) for c in plan[1:5]] == [(t - 24, 24), (t + 2 * 24, -24), (t + 24, 24), (t + 5 * 24, -24)]
    for (base, step), rows in zip([gaps.stacked(stack, c) for c in plan[1:5]], ([0, 1], [1, 0], [2, 3, 4], [4, 3, 2])):
        assert [base + s * step for s in range(1, len(rows) + 1)] == [stack[r].data_ptr() for r in rows]
    assert gaps.fixed(stack, 3) == (t + 3 * 24, 0)
