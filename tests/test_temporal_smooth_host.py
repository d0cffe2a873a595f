"""The video temporal smooth, the parts that need no device: the properties the rule promises on the restatement
(tests/temporal_smooth_ref.py) as bits and counts, the C entry's argument checks (made before any HIP call), the wrappers'
argument checks, the node's protocol and the no-fallback errors.  Layouts, constants and names against the header are
tests/test_cabi_mirror.py's, for the whole C ABI."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi
from tests import temporal_smooth_ref as sref
from tests.compare import _f32_bits as _bits
from tests.temporal_clips import (NOISE_RATIO, RADII, check_outside, check_smooth_ghost as check_ghost, check_smooth_noise as check_noise,
                                  check_smooth_pan as check_pan, ghost_clip, noise_clip, smooth_pan_clip as pan_clip,
                                  smooth_still_clip as still_clip)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the properties, on the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("motion", sref.MOTIONS)
@pytest.mark.parametrize("radius", RADII)
def test_pan_with_alternating_flicker_is_recovered_bit_for_bit(radius, motion):
    _, clip, mask = pan_clip()
    check_pan(radius, motion, *sref.temporal_smooth_ref(clip, mask, radius, 24, motion))


@pytest.mark.parametrize("radius", RADII)
def test_noise_variance_falls_as_the_weights_say(radius):
    _, clip, mask = noise_clip()
    check_noise(radius, *sref.temporal_smooth_ref(clip, mask, radius, 24))


def test_an_object_beyond_the_tolerance_leaves_no_ghost():
    clip, mask = ghost_clip()
    check_ghost(*sref.temporal_smooth_ref(clip, mask, 2, 24))


def test_one_frame_an_empty_mask_and_a_still_clip_return_the_images():
    _, clip, mask = noise_clip()
    out, support = sref.temporal_smooth_ref(clip[:1], mask, 2, 24)
    assert (_bits(out) == _bits(clip[:1])).all() and (support[0] == np.where(mask == 1, 0, -1)).all()
    out, support = sref.temporal_smooth_ref(clip, np.zeros_like(mask), 2, 24)
    assert (_bits(out) == _bits(clip)).all() and (support == -1).all()
    still, mask = still_clip()
    for motion in sref.MOTIONS:
        out, support = sref.temporal_smooth_ref(still, mask, 3, 24, motion)
        assert (_bits(out) == _bits(still)).all()
        assert (support[4][mask == 1] == 6).all() and (support[0][mask == 1] == 3).all() and (support[7][mask == 1] == 4).all()
    negative = -still                                                  # -x + 0 / W keeps the sign bit of every value too
    out, _ = sref.temporal_smooth_ref(negative, mask, 2, 0)
    assert (_bits(out) == _bits(negative)).all()


def test_tolerance_zero_leaves_a_noisy_clip_and_the_outside_never_changes():
    # tolerance 0 accepts a sample only when every channel has the pixel's own code; under noise of 15 codes none of the 8640 has
    still, mask = still_clip()
    loud = still.copy()
    loud[:, mask == 1] += np.random.default_rng(9).normal(0, 0.06, (still.shape[0], int(mask.sum()), 3)).astype(np.float32)
    out, support = sref.temporal_smooth_ref(loud, mask, 2, 0)
    check_outside(loud, mask, out, support)
    assert (_bits(out) == _bits(loud)).all() and (support[:, mask == 1] == 0).all()
    _, clip, mask = noise_clip()
    out, support = sref.temporal_smooth_ref(clip, mask, 2, 255)
    check_outside(clip, mask, out, support)
    assert (support[2:7][:, mask == 1] == 4).all() and (_bits(out) != _bits(clip))[:, mask == 1].any()


def test_a_nan_sample_that_is_accepted_makes_the_pixel_nan_and_a_nan_mask_is_known():
    still, mask = still_clip()
    clip = still.copy()
    clip[3, 12, 16] = np.nan                                           # code 0: 64 or more away from the canvas, rejected
    out, support = sref.temporal_smooth_ref(clip, mask, 1, 24)
    assert (_bits(out) == _bits(clip)).all() and support[3, 12, 16] == 0 and support[2, 12, 16] == 1
    out, support = sref.temporal_smooth_ref(clip, mask, 1, 255)
    assert np.isnan(out[2:5, 12, 16]).all() and not np.isnan(out[[1, 5], 12, 16]).any() and support[2, 12, 16] == 2
    holes = mask.copy()
    holes[11, 15] = np.nan
    assert sref.temporal_smooth_ref(clip, holes, 1, 24)[1][0, 11, 15] == -1


def test_weights_are_the_binomial_row():
    assert sref.weights(1) == [2, 1] and sref.weights(2) == [6, 4, 1] and sref.weights(8)[0] == 12870
    for radius in range(1, _cabi.LP_TSMOOTH_MAX_RADIUS + 1):
        w = sref.weights(radius)
        assert w[0] + 2 * sum(w[1:]) == 4 ** radius <= 65536
    for radius in RADII:
        w = sref.weights(radius)
        assert NOISE_RATIO[radius] == (w[0] ** 2 + 2 * sum(v * v for v in w[1:])) / 16 ** radius


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_entry_rejects_bad_arguments_without_a_device(hip_lib):
    C, E, U = ctypes, _cabi.LP_E_INVALID, _cabi.LP_E_UNSUPPORTED
    side = _cabi.LP_VMASK_MAX_SIDE
    a = [C.c_void_p(4096 * (i + 1)) for i in range(8)]                # never dereferenced: validation comes before any HIP call
    names = [f for f, t in _cabi.LpTsmoothDesc._fields_ if t is C.c_void_p]
    assert names == ["fwd", "bwd", "known", "images", "out", "support"]
    # frames 3 .. 5 of 10 with radius 2: fwd of 3 .. 6, bwd of 2 .. 5
    good = dict(frames=10, height=40, width=70, channels=3, first=3, count=3, radius=2, tolerance=24, fwd_first=3, fwd_count=4,
                bwd_first=2, bwd_count=4, known_stride=40 * 70, **dict(zip(names, a)))

    def call(**change):
        return hip_lib.lp_tsmooth(C.byref(_cabi.LpTsmoothDesc(**{**good, **change})), None)
    assert hip_lib.lp_tsmooth(None, None) == E
    for change in ({"frames": 0}, {"frames": -1}, {"height": 0}, {"height": side + 1}, {"width": 0}, {"width": side + 1},
                   {"channels": 0}, {"channels": _cabi.LP_DETAIL_MAX_CHANNELS + 1}, {"radius": 0}, {"radius": _cabi.LP_TSMOOTH_MAX_RADIUS + 1},
                   {"tolerance": -1}, {"tolerance": 256}, {"first": -1}, {"first": 10}, {"count": 0}, {"count": 8}, {"count": -1},
                   {"fwd_first": 4}, {"fwd_first": -1}, {"fwd_count": 3}, {"fwd_count": 0}, {"bwd_first": 3}, {"bwd_first": -1},
                   {"bwd_count": 3}, {"bwd_count": 0}, {"known_stride": 40 * 70 - 1}, {"known_stride": -1}, {"radius": 3}):
        assert call(**change) == E, change
    for name in names:
        assert call(**{name: None}) == E, name
    for out in ("out", "support"):                                     # an output that is an input or the other output
        for other in names:
            if other != out:
                assert call(**{out: good[other]}) == E, (out, other)
    assert call(frames=65536) == U


def test_the_header_and_the_documents_say_the_smooth_words():
    read = lambda *path: open(os.path.join(ROOT, *path)).read()       # noqa: E731
    header = read("include", "lanpaint_hip.h")
    assert "temporal_smooth_kernel.hip" in read("lanpaint_amd", "build.py")
    for word in ("LP_TSMOOTH_MAX_RADIUS", "w_k = C(2R, R + k)", "keeps x bit for bit", "a tap with weight 0 is not", "no FMA",
                 "an accepted NaN sample makes that pixel NaN", "for every chunking", "a single outlier frame", "support = -1"):
        assert word in header, word
    for doc in ("README.md", "DESIGN.md", "CHANGES.md", "INTEGRATION.md"):
        text = read(doc)
        assert "LanPaint_VideoTemporalSmooth" in text and "temporal_smooth" in text, doc
    assert re.search(r"VideoTemporalSmooth\s*->\s*(LanPaint_)?MultibandBlend", read("INTEGRATION.md"))


# ---- the wrappers and the node ----------------------------------------------------------------------------------------------------------
def test_temporal_smooth_refuses_cpu_tensors_and_bad_arguments():
    from lanpaint_amd import temporal_smooth as ts
    images, mask = torch.zeros(4, 16, 16, 3), torch.zeros(4, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ts.temporal_smooth(images, mask)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ts.temporal_smooth(images.numpy(), mask)
    fields = torch.zeros(3, 2, 2, 2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ts.smooth_frames(fields, fields, torch.zeros(4, 16, 16, dtype=torch.uint8), images)
    # the numbers are checked before the tensors are looked at
    for bad in (dict(radius=0), dict(radius=9), dict(radius=2.0), dict(radius=True), dict(tolerance=-1), dict(tolerance=256),
                dict(tolerance=24.0), dict(motion="subject"), dict(motion=None), dict(levels=0), dict(levels=7), dict(search=0),
                dict(search=8), dict(smooth=-1), dict(smooth=65)):
        with pytest.raises(ValueError):
            ts.temporal_smooth(images, mask, **bad)
    for bad in (dict(radius=0), dict(radius=9), dict(tolerance=-1), dict(tolerance=256)):
        with pytest.raises(ValueError):
            ts.smooth_frames(fields, fields, torch.zeros(4, 16, 16, dtype=torch.uint8), images, **bad)
    assert ts.WS_CAP_BYTES == 1 << 30 and ts.MAX_RADIUS == 8 and ts.MOTIONS == sref.MOTIONS
    # frames 3 .. 5 of 10 with radius 2 read fwd of 3 .. 6 and bwd of 2 .. 5; the clip's ends cut both
    assert [list(r) for r in ts.field_steps(3, 6, 10, 2)] == [[3, 4, 5, 6], [2, 3, 4, 5]]
    assert [list(r) for r in ts.field_steps(0, 10, 10, 8)] == [list(range(9)), list(range(1, 10))]
    assert [list(r) for r in ts.field_steps(0, 1, 1, 3)] == [[], []]
    assert [list(r) for r in ts.field_steps(9, 10, 10, 1)] == [[], [9]]


def test_node_protocol_and_own_mappings():
    from lanpaint_amd import temporal_smooth_nodes
    node = temporal_smooth_nodes.LanPaint_VideoTemporalSmooth
    assert temporal_smooth_nodes.NODE_CLASS_MAPPINGS == {"LanPaint_VideoTemporalSmooth": node}
    assert list(temporal_smooth_nodes.NODE_DISPLAY_NAME_MAPPINGS) == ["LanPaint_VideoTemporalSmooth"]
    types = node.INPUT_TYPES()
    req = types["required"]
    assert list(types) == ["required"]
    assert list(req) == ["image", "mask", "radius", "tolerance", "motion", "levels", "search", "smooth"]
    assert req["image"][0] == "IMAGE" and req["mask"][0] == "MASK"
    assert req["radius"][0] == "INT" and req["radius"][1] == {**req["radius"][1], "default": 2, "min": 1, "max": 8}
    assert req["tolerance"][0] == "INT" and req["tolerance"][1] == {**req["tolerance"][1], "default": 24, "min": 0, "max": 255}
    assert req["motion"][0] == ["background", "picture"] and req["motion"][1]["default"] == "background"
    assert req["levels"][0] == "INT" and req["levels"][1] == {**req["levels"][1], "default": 4, "min": 1, "max": 6}
    assert req["search"][0] == "INT" and req["search"][1] == {**req["search"][1], "default": 2, "min": 1, "max": 7}
    assert req["smooth"][0] == "INT" and req["smooth"][1] == {**req["smooth"][1], "default": 8, "min": 0, "max": 64}
    for name in req:
        assert len(req[name][1]["tooltip"]) > 20, name
    for word in ("boiling", "motion", "neighbouring frames", "tolerance", "multiband blend", "grain", "support", "outlier"):
        assert word in node.DESCRIPTION, word
    assert node.RETURN_TYPES == ("IMAGE", "MASK") and node.RETURN_NAMES == ("image", "support")
    assert node.FUNCTION == "smooth" and callable(getattr(node, node.FUNCTION))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            node().smooth(torch.zeros(3, 16, 16, 3), torch.zeros(3, 16, 16))
