"""Device plumbing the GPU tests share: the device, host-to-device copies, level counts, the calibrated spin delay."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, propagate


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return _cabi.load()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


DEV = torch.device("cuda", 0)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# How long the side stream is held back, in milliseconds.  It has to outlast the host's side of the call.  Measured on the MI355X
# (the warm call of each of the ten on (23, 33), whole mode, poison 0xFF, host wall time in ms; the first call on a stream, which
# loads kernels and fills the allocator's pool, is not the warm one: it took up to 208 ms):
#     propagate_masks 0.68, propagate_masks_visible 0.86, propagate_masks_anchored 0.92, propagate_keys 0.57,
#     propagate_keys_visible 0.76, temporal_fill 0.56, temporal_fill_checked 0.83, temporal_smooth 0.33,
#     temporal_smooth_robust 0.29, detect_shots 0.11
# The largest is 0.92 ms (0.87 in another run).  The host side of ~100 ctypes launches jitters and the test machine is shared, so the delay is not 4 x
# but more than 100 x that, and still well under a second: the ten tests spend one second waiting in all.
DELAY_MS = 100


@functools.lru_cache(maxsize=None)
def _spin_cycles_per_ms():
    """What `torch.cuda._sleep` counts in a millisecond on this device, measured once with events on the default stream."""
    torch.cuda._sleep(1000)                                            # the kernel's first launch loads it
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cycles = 20_000_000
    a.record()
    torch.cuda._sleep(cycles)
    b.record()
    b.synchronize()
    return cycles / a.elapsed_time(b)


def _levels_of(pyr, H, W, levels):
    """The device's frame pyramids uint8 [n, stride] as one numpy array per level."""
    host = pyr.cpu()
    return [propagate.level_view(host, H, W, lv).numpy() for lv in range(levels)]


def _equal(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want), what


def _match_jobs(rows):
    arr = (_cabi.LpPropMatchJob * len(rows))(*[_cabi.LpPropMatchJob(*r) for r in rows])
    return arr, ctypes.cast(arr, ctypes.c_void_p)
