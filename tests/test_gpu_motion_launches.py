"""The launch sequences of the motion family: the ordered C entry names each of the nine public calls issues on a tiny clip are
those recorded before the nine modules got their shared host layer (lanpaint_amd/_motion.py).  Names only; the bits are the
other suites' business.  tests/golden/motion_launches.json holds them, once with every cap as it is ("whole", fp32 images) and
once with each module's WS_CAP_BYTES lowered so that a chunk holds one or two frames ("chunked", fp16 images, so the
conversions go in chunks too)."""
from __future__ import annotations

import json
import os

import pytest
import torch

from lanpaint_amd import (_cabi, propagate, propagate_keys, propagate_keys_visible, propagate_visible, shots, temporal_fill,
                          temporal_fill_checked, temporal_smooth, temporal_smooth_robust)
from tests.device import _dev
from tests.helpers import GOLDEN_DIR, record_launches
from tests.inputs import _disc, _video

pytestmark = pytest.mark.gpu
MODULES = (propagate, propagate_visible, propagate_keys, propagate_keys_visible, temporal_fill, temporal_fill_checked, temporal_smooth,
           temporal_smooth_robust, shots)
F, H, W = 5, 24, 40
LEVELS, SEARCH, SMOOTH, KEY, KEYS, RADIUS = 3, 2, 8, 2, [0, 4], 2


def _lower_caps(monkeypatch):
    stride = _cabi.prop_pyramid_ws_bytes(1, H, W, LEVELS)
    gh, gw = _cabi.prop_grid(H, W)
    plane, cells = H * W * 4, gh * gw * 4
    monkeypatch.setattr(propagate, "WS_CAP_BYTES", 2 * stride + 8)                    # a frame and its fp32 copy: one frame a chunk
    monkeypatch.setattr(propagate_keys, "WS_CAP_BYTES", F * stride + 8)               # the clip's pyramids; a frame a conversion
    monkeypatch.setattr(propagate_keys_visible, "WS_CAP_BYTES", 9 * (plane + cells))  # what it keeps for one gap of 3 frames, 2 chains
    monkeypatch.setattr(temporal_fill, "WS_CAP_BYTES", 2 * stride + 2 * (2 * stride + gh * gw * 8) + 8)       # two steps a chunk
    monkeypatch.setattr(temporal_smooth, "WS_CAP_BYTES", (2 * RADIUS + 1) * (2 * stride + 2 * gh * gw * 8) + 8)   # one frame a chunk
    monkeypatch.setattr(shots, "WS_CAP_BYTES", 1)                                     # one pair a chunk


def launch_lists(monkeypatch, names):
    """{"whole" | "chunked": {call: [entry names]}}; `names` is the list the patched launches append to."""
    images, mask = _dev(_video(F, H, W, 3)), _dev(_disc(H, W))
    out = {}
    for mode in ("whole", "chunked"):
        if mode == "chunked":
            _lower_caps(monkeypatch)
            images = images.half()
        keys = mask[None].repeat(len(KEYS), 1, 1)
        calls = {
            "propagate_masks": lambda: propagate.propagate_masks(images, mask, KEY, LEVELS, SEARCH, SMOOTH),
            "propagate_masks_visible": lambda: propagate_visible.propagate_masks_visible(images, mask, KEY, LEVELS, SEARCH, SMOOTH),
            "propagate_keys": lambda: propagate_keys.propagate_keys(images, keys, KEYS, LEVELS, SEARCH, SMOOTH),
            "propagate_keys_visible": lambda: propagate_keys_visible.propagate_keys_visible(images, keys, KEYS, LEVELS, SEARCH, SMOOTH),
            "temporal_fill": lambda: temporal_fill.temporal_fill(images, mask, LEVELS, SEARCH, SMOOTH),
            "temporal_fill_checked": lambda: temporal_fill_checked.temporal_fill_checked(images, mask, LEVELS, SEARCH, SMOOTH),
            "temporal_smooth": lambda: temporal_smooth.temporal_smooth(images, mask, RADIUS, 24, "background", LEVELS, SEARCH, SMOOTH),
            "temporal_smooth_robust": lambda: temporal_smooth_robust.temporal_smooth_robust(images, mask, RADIUS, 24, "background",
                                                                                            LEVELS, SEARCH, SMOOTH),
            "detect_shots": lambda: shots.detect_shots(images),
        }
        out[mode] = {}
        for call, fn in calls.items():
            del names[:]
            fn()
            out[mode][call] = list(names)
    torch.cuda.synchronize()
    return out


def test_the_nine_calls_issue_the_recorded_launches(monkeypatch):
    with open(os.path.join(GOLDEN_DIR, "motion_launches.json")) as f:
        want = json.load(f)
    got = launch_lists(monkeypatch, record_launches(monkeypatch, *MODULES))
    assert sorted(got) == sorted(want)
    for mode in want:
        assert sorted(got[mode]) == sorted(want[mode]) and len(want[mode]) == 9
        for call in want[mode]:
            assert got[mode][call] == want[mode][call], (mode, call)
