"""The motion modules' shared host layer (lanpaint_amd/_motion.py, and `tensor_is` in _hostcall.py) where no device is needed: the
checks' messages, and the job tables of the field walk against addresses worked out by hand.  The device rule is switched off
for the checks behind it; the walk runs on host memory with its launches recorded instead of made."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, _hostcall, _motion

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
    """What `temporal_fill.step_fields` and `propagate_keys._Chains._bind` wrote into their tables before the walk was shared: per
    level a match row (source, target, weights, the level above's field or 0, raw, valid) and a fill row (raw, valid, field), the
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
