"""tests/poison.py on CPU tensors: what a poisoned `torch.empty` / `torch.empty_like` hands out, what it leaves alone, and that the
real functions are back when the test that asked for it has ended.  No device."""
import pytest
import torch

from tests.poison import poisoned_empty

REAL = (torch.empty, torch.empty_like)


def test_ff_reads_as_minus_one_255_and_nan(monkeypatch):
    filled = poisoned_empty(monkeypatch, 0xFF)
    assert torch.empty is not REAL[0] and torch.empty_like is not REAL[1]
    i = torch.empty((3, 5), dtype=torch.int32)
    assert i.dtype == torch.int32 and tuple(i.shape) == (3, 5) and (i == -1).all()
    assert (torch.empty(7, dtype=torch.uint8) == 255).all()
    assert (torch.empty((2, 3), dtype=torch.int64) == -1).all()
    f = torch.empty((4, 2, 3))
    assert f.dtype == torch.float32 and torch.isnan(f).all()
    assert (f.view(torch.int32) == -1).all()                            # every byte, not a NaN of some other pattern
    assert torch.isnan(torch.empty(5, dtype=torch.float16)).all()
    assert torch.empty((2, 2), dtype=torch.bool).view(torch.uint8).eq(255).all()
    like = torch.empty_like(torch.zeros((2, 9)))                        # does not go through torch.empty: patched on its own
    assert like.dtype == torch.float32 and tuple(like.shape) == (2, 9) and torch.isnan(like).all()
    assert (torch.empty_like(torch.zeros(4, dtype=torch.int32)) == -1).all()
    assert (torch.empty_like(torch.zeros(4), dtype=torch.uint8) == 255).all()
    assert filled == [60, 7, 48, 96, 10, 4, 72, 16, 4]


def test_00_reads_as_zero_and_other_bytes_as_themselves(monkeypatch):
    poisoned_empty(monkeypatch, 0x00)
    assert (torch.empty((3, 5), dtype=torch.int32) == 0).all()
    assert (torch.empty((3, 5)).view(torch.int32) == 0).all()
    assert (torch.empty_like(torch.ones(6)).view(torch.int32) == 0).all()
    monkeypatch.undo()
    poisoned_empty(monkeypatch, 0x5A)
    assert (torch.empty(9, dtype=torch.uint8) == 0x5A).all()
    assert (torch.empty(2, dtype=torch.int32) == 0x5A5A5A5A).all()


def test_the_eight_byte_types_read_as_minus_one_nan_and_zero(monkeypatch):
    """int64 and float64, which the image-space family allocates through it (the grain tables and the EDT's centroid sums, the
    colour match's workspace and table, the EDT's SDF): every one of the eight bytes holds the poison."""
    filled = poisoned_empty(monkeypatch, 0xFF)
    i, f = torch.empty((2, 3, 8, 3), dtype=torch.int64), torch.empty((3, 13), dtype=torch.float64)
    assert i.dtype == torch.int64 and tuple(i.shape) == (2, 3, 8, 3) and (i == -1).all()
    assert f.dtype == torch.float64 and tuple(f.shape) == (3, 13) and torch.isnan(f).all() and (f.view(torch.int64) == -1).all()
    assert (torch.empty_like(i) == -1).all() and torch.isnan(torch.empty_like(f)).all()
    assert filled == [1152, 312, 1152, 312]
    monkeypatch.undo()
    filled = poisoned_empty(monkeypatch, 0x00)
    i, f = torch.empty((2, 3, 8, 3), dtype=torch.int64), torch.empty((3, 13), dtype=torch.float64)
    assert (i == 0).all() and (f == 0).all() and (f.view(torch.int64) == 0).all()                # +0.0, not -0.0
    assert (torch.empty_like(i) == 0).all() and (torch.empty_like(f).view(torch.int64) == 0).all()
    assert filled == [1152, 312, 1152, 312]


def test_a_tensor_without_elements_survives_and_zeros_is_not_touched(monkeypatch):
    filled = poisoned_empty(monkeypatch, 0xFF)
    for shape in ((0,), (0, 2), (3, 0, 5)):
        t = torch.empty(shape, dtype=torch.int64)
        assert tuple(t.shape) == shape and t.numel() == 0
        assert torch.empty_like(t).numel() == 0
    assert filled == []
    z = torch.zeros((3, 4))
    assert (z.view(torch.int32) == 0).all()
    assert (torch.zeros_like(torch.ones(5)) == 0).all() and (torch.ones(3) == 1).all() and (torch.full((2,), 7) == 7).all()
    assert filled == []                                                # none of them went through the wrappers


def test_keyword_arguments_pass_through(monkeypatch):
    poisoned_empty(monkeypatch, 0xFF)
    t = torch.empty(size=(2, 3), dtype=torch.int16, device="cpu")
    assert t.dtype == torch.int16 and t.device.type == "cpu" and (t == -1).all()
    out = torch.zeros(4, dtype=torch.int32)
    assert torch.empty(4, dtype=torch.int32, out=out) is out and (out == -1).all()


def test_a_byte_outside_0_to_255_is_refused(monkeypatch):
    for bad in (-1, 256, 1.0, None):
        with pytest.raises(ValueError):
            poisoned_empty(monkeypatch, bad)
    assert (torch.empty, torch.empty_like) == REAL


def test_the_real_functions_are_back_after_the_tests_above():
    assert (torch.empty, torch.empty_like) == REAL
    assert torch.empty((2, 2)).shape == (2, 2)
