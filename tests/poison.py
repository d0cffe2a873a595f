"""Poisoned allocations for the tests: while a test runs, every tensor that `torch.empty` or `torch.empty_like` hands out holds a
chosen byte in every position.  The caching allocator gives a call the block the last call of the same shape released, which very
often holds the right answer already; a kernel that reads a cell before it writes it, skips an output element or lets padding reach
a result passes on such a block.  Under a poison the element shows: 0x00 reads as integer 0, 0.0 and flag false, 0xFF as integer
-1, NaN, flag true and byte 255.  Not a conftest: a test asks for it by name.  POISONS and poison_id parametrise the scratch tests."""
import torch


def poisoned_empty(monkeypatch, byte):
    """Replace `torch.empty` and `torch.empty_like` (which does not go through the Python-level `torch.empty`) until the test ends:
    each calls the real function and fills the result's bytes with `byte` on the current stream.  A tensor without elements is
    left alone.  Any device.  Returns the list the wrappers append every poisoned tensor's byte count to, so that a test can tell
    that the code under it did allocate through them."""
    if not isinstance(byte, int) or not 0 <= byte <= 255:
        raise ValueError(f"byte must be an integer in 0..255, got {byte!r}")
    filled = []

    def poisoned(real):
        def wrapper(*args, **kwargs):
            t = real(*args, **kwargs)
            if t.numel():
                t.view(torch.uint8).fill_(byte)
                filled.append(t.numel() * t.element_size())
            return t
        wrapper.__name__, wrapper.__doc__ = real.__name__, real.__doc__
        return wrapper

    monkeypatch.setattr(torch, "empty", poisoned(torch.empty))
    monkeypatch.setattr(torch, "empty_like", poisoned(torch.empty_like))
    return filled


POISONS = [0x00, 0xFF]
poison_id = lambda b: f"0x{b:02X}"                                   # noqa: E731
