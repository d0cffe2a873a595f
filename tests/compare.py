"""Comparisons the tests share: bit views of arrays and the exact-equality checks built on them.  numpy only, no device."""
import numpy as np


def ulps(a, b):
    """Distance in fp32 units in the last place (of the larger magnitude)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def _tensor_bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _raw_bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_typed(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    bad = (_raw_bits(got) != _raw_bits(want)) if got.dtype == np.float32 else (got != want)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def _f32_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_ints(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.astype(np.int64) != want.astype(np.int64)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def _same_bits(got, want, what):
    assert got.dtype == np.float32 and got.shape == want.shape, what
    bad = _f32_bits(got) != _f32_bits(want)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def _same_raw_bits(got, want, what):
    assert got.dtype == np.float32 and got.shape == want.shape, what
    bad = _raw_bits(got) != _raw_bits(want)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def _same_values(got, want, what):
    """fp32: NaN where the restatement has NaN, else the same bits."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    nan = np.isnan(want)
    bad = (np.isnan(got) != nan) | (~nan & (_f32_bits(got) != _f32_bits(want)))
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def _iou(a, b):
    return float((a & b).sum()) / max(int((a | b).sum()), 1)
