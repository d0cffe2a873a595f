"""The anchored occlusion-aware video mask propagate on the MI355X where its own suite does not look, as
tests/test_gpu_motion_scratch.py does it for the rest of the motion family, whose helpers this uses: scratch and outputs that hold
a poison before the call, and a side stream that is held back while the call is made.  Every comparison is bit for bit against the
numpy restatement."""
import time

import pytest
import torch

from lanpaint_amd import propagate, propagate_anchored, propagate_anchored_visible, propagate_visible
from tests import device, inputs, motion_checks
from tests import propagate_anchored_visible_ref as avref
from tests.compare import _same_bits, _same_ints as _same
from tests.device import DELAY_MS, _spin_cycles_per_ms
from tests.helpers import record_launches
from tests.inputs import SMALL
from tests.poison import POISONS, poison_id, poisoned_empty

pytestmark = pytest.mark.gpu
FRAMES, KEY = 7, 3            # the key in the middle: three steps either way, so both buffers of every ping-pong pair are written and read


def _call():
    """(the device's inputs, the restatement's (mask, hidden)) of the suite's 7-frame clip on (23, 33), at 3 levels."""
    images, truth = inputs._anchored_visible_clip(FRAMES, *SMALL, KEY)
    return (device._dev(images), device._dev(truth[KEY].astype("float32"))), inputs._anchored_visible_want(FRAMES, *SMALL, KEY)[0]


def _compare(got, want, what):
    assert len(got) == len(want) == 2
    for g, w, name in zip(got, want, ("mask", "hidden")):
        assert g.is_cuda and g.dtype == torch.float32
        _same_bits(g.cpu().numpy(), w, (what, name))


@pytest.mark.parametrize("poison", POISONS, ids=poison_id)
@pytest.mark.parametrize("mode", ["whole", "chunked"])
def test_the_call_under_poison_equals_the_restatement(mode, poison, monkeypatch):
    (images, mask), want = _call()
    if mode == "chunked":                                              # fp32 images need no copy: one frame's pyramid a chunk
        monkeypatch.setattr(propagate, "WS_CAP_BYTES", propagate._cabi.prop_pyramid_ws_bytes(1, *SMALL, inputs.ANCHORED_VISIBLE_LEVELS) + 8)
    names = record_launches(monkeypatch, propagate_anchored_visible, propagate_anchored, propagate_visible, propagate)
    filled = poisoned_empty(monkeypatch, poison)
    got = motion_checks._anchored_visible_call(images, mask, KEY)
    assert filled                                                      # the call's buffers did come through the poison
    lumas = names.count("lp_prop_luma")
    assert lumas <= 2 if mode == "whole" else lumas >= 5, (mode, lumas)
    assert names.count("lp_prop_anchor_match_gated") == FRAMES - 1
    _compare(got, want, (mode, poison_id(poison)))


@pytest.mark.parametrize("poison", POISONS, ids=poison_id)
def test_gated_anchor_field_under_poison(poison, monkeypatch):
    filled = poisoned_empty(monkeypatch, poison)
    for positions, lumas, mask, occlusion in (("smooth", "noisy", "disc", 16), ("outside", "dark", "random", 1), ("key", "noisy", "full", 16),
                                              ("key", "noisy", "empty", 16)):
        P, Yt, Yk, m = inputs._anchored_visible_inputs(SMALL, positions, lumas, mask)
        want_vec, want_valid, want_gated = avref.gated_anchor_field(P, Yt, Yk, m, 2, 8, occlusion)
        vec, valid, gated = motion_checks._anchored_visible_field(P, Yt, Yk, m, 2, 8, occlusion)
        _same(gated, want_gated, ("gated", positions, lumas, mask))
        _same(valid, want_valid, ("valid", positions, lumas, mask))
        _same(vec, want_vec, ("vec", positions, lumas, mask))
    assert filled


def test_the_call_on_a_held_back_side_stream_reads_nothing_back(monkeypatch):
    """tests/test_gpu_motion_scratch.py's test of the same name, for this call: made on a side stream behind a queued delay, the
    call returns before the delay is done (no device -> host read, no synchronisation), leaves nothing on the null stream, and
    every launch waits behind the poison fills of its buffers on that stream, or the bits differ."""
    (images, mask), want = _call()                                     # built on the default stream
    cycles = int(_spin_cycles_per_ms() * DELAY_MS)
    torch.cuda.synchronize()
    filled = poisoned_empty(monkeypatch, 0xFF)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        motion_checks._anchored_visible_call(images, mask, KEY)                                # the first call loads the kernels and fills the allocator's
        side.synchronize()                                             # pool of this stream: no hipMalloc below
        del filled[:]
        done = torch.cuda.Event()
        torch.cuda._sleep(cycles)
        done.record(side)
        start = time.perf_counter()
        got = motion_checks._anchored_visible_call(images, mask, KEY)
        held = not done.query()                                        # directly behind the call, before anything synchronises
        idle = torch.cuda.default_stream().query()
        call_ms = (time.perf_counter() - start) * 1e3
    print(f"propagate_masks_anchored_visible: call behind the delay {call_ms:.2f} ms of host time; delay {DELAY_MS} ms")
    assert held, (f"the call returned after {call_ms:.2f} ms with the {DELAY_MS} ms delay in front of it done: it waited for the "
                  "device, or the delay is too short for this host")
    assert idle, "the call left work on the null stream"
    assert filled
    side.synchronize()
    _compare(got, want, "side stream")
