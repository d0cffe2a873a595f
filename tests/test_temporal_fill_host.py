"""The video temporal fill, the parts that need no device: the properties the rule promises on the restatement
(tests/temporal_fill_ref.py) as bits and counts, the C entries' argument checks (made before any HIP call), the wrappers' argument
checks, the node's protocol and the no-fallback errors.  Layouts, constants and names against the header are
tests/test_cabi_mirror.py's, for the whole C ABI."""
import ctypes
import os

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi
from tests import propagate_ref as ref
from tests import temporal_fill_ref as tref
from tests.compare import _f32_bits as _bits
from tests.temporal_clips import (STILL_REMAINING, check_fill_fixed as check_fixed, check_fill_pan as check_pan,
                                  check_fill_still as check_still, fill_pan_clip as pan_clip, fill_still_clip as still_clip)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the properties, on the restatement ---------------------------------------------------------------------------------------------------
def test_pan_clip_is_filled_with_the_true_background_bit_for_bit():
    _, clip, mask = pan_clip()
    check_pan(*tref.temporal_fill_ref(clip, mask))


@pytest.mark.parametrize("reach", list(STILL_REMAINING))
def test_reach_bounds_the_age_on_a_still_canvas(reach):
    _, clip, mask = still_clip(2)
    check_still(reach, *tref.temporal_fill_ref(clip, mask, reach=reach))


def test_a_fixed_subject_stays_in_remaining():
    _, clip, mask = still_clip(0)
    check_fixed(*tref.temporal_fill_ref(clip, mask))


def test_one_frame_empty_and_full_masks_return_the_images_and_a_tie_stays_with_the_past():
    rng = np.random.default_rng(7)
    video = rng.random((4, 16, 17, 3), dtype=np.float32)
    soft = rng.random((4, 16, 17), dtype=np.float32)
    filled, remaining, source = tref.temporal_fill_ref(video[:1], soft[:1], 3)
    assert (_bits(filled) == _bits(video[:1])).all() and (remaining[0] == ref.binarise(soft[0])).all()
    for value in (0.0, 1.0):
        filled, remaining, source = tref.temporal_fill_ref(video, np.full((16, 17), value, np.float32), 3)
        assert (_bits(filled) == _bits(video)).all() and (remaining == value).all()
        assert (source == (np.arange(4)[:, None, None] if value == 0 else -1)).all()
    # frame 1 of three equal frames, masked there only: both neighbours show it at age 1, the earlier one is taken
    still = np.repeat(video[:1], 3, axis=0)
    mask = np.zeros((3, 16, 17), np.float32)
    mask[1, 4:9, 5:12] = 1
    filled, remaining, source = tref.temporal_fill_ref(still, mask, 3)
    assert not remaining.any() and (source[1][mask[1] == 1] == 0).all() and (_bits(filled) == _bits(still)).all()
    # a NaN in the mask is known; a non-finite neighbour of a whole-pixel origin does not leak
    wild = still.copy()
    wild[:, 3, :] = np.nan
    wild[:, :, 4] = np.inf
    filled, _, _ = tref.temporal_fill_ref(wild, mask, 3)
    assert (_bits(filled) == _bits(wild)).all()


def test_the_sample_one_value_at_a_time():
    img = np.zeros((1, 2, 2, 1), np.float32)
    img[0, :, :, 0] = [[1, 3], [5, 9]]
    one = lambda y, x: tref.sample(img, np.array([0]), np.array([y]), np.array([x]))[0, 0]    # noqa: E731
    assert one(0, 0) == 1 and one(0, 16) == 3 and one(16, 0) == 5 and one(16, 16) == 9
    assert one(0, 8) == 2 and one(8, 0) == 3 and one(8, 8) == np.float32(4.5) and one(4, 12) == np.float32(((4 * 1 + 12 * 3) * 12 + (4 * 5 + 12 * 9) * 4) / 256)
    assert one(-5, 40) == 3 and one(99, -1) == 5                       # clamped to the plane
    img[0, 1, 1, 0] = np.nan
    assert one(0, 0) == 1 and one(0, 16) == 3 and one(16, 0) == 5 and np.isnan(one(1, 1))


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_entries_reject_bad_arguments_without_a_device(hip_lib):
    C, E, U = ctypes, _cabi.LP_E_INVALID, _cabi.LP_E_UNSUPPORTED
    side = _cabi.LP_VMASK_MAX_SIDE
    a = [C.c_void_p(4096 * (i + 1)) for i in range(12)]               # never dereferenced: validation comes before any HIP call

    good = dict(frames=5, height=40, width=70, levels=3, mask_frames=5, mask=a[0], pyramid=a[1], source=a[2], remaining=a[3])
    assert hip_lib.lp_tfill_known(None, None) == E
    for change in ({"frames": 0}, {"frames": -1}, {"height": 0}, {"height": side + 1}, {"width": 0}, {"width": side + 1},
                   {"levels": 0}, {"levels": _cabi.LP_PROP_MAX_LEVELS + 1}, {"mask_frames": 0}, {"mask_frames": 2}, {"mask_frames": 6},
                   {"frame0": -1},
                   {"mask": None}, {"pyramid": None}, {"pyramid": a[0]}, {"source": a[0]}, {"remaining": a[0]}, {"source": a[1]},
                   {"remaining": a[1]}, {"remaining": a[2]}):
        assert hip_lib.lp_tfill_known(C.byref(_cabi.LpTfillKnownDesc(**{**good, **change})), None) == E, change
    assert hip_lib.lp_tfill_known(C.byref(_cabi.LpTfillKnownDesc(**{**good, "frames": 65536, "mask_frames": 1})), None) == U
    assert hip_lib.lp_tfill_known(C.byref(_cabi.LpTfillKnownDesc(**{**good, "frames": 65536, "mask_frames": 65536})), None) == U
    assert hip_lib.lp_tfill_known(C.byref(_cabi.LpTfillKnownDesc(**{**good, "frame0": 65531})), None) == U      # frame 65535 would be its last

    names = [f for f, t in _cabi.LpTfillCarryDesc._fields_ if t is C.c_void_p]
    good = dict(frames=5, height=40, width=70, channels=3, frame=2, donor=1, reach=0, nearer=0, **dict(zip(names, a)))
    assert len(names) == 11 and hip_lib.lp_tfill_carry(None, None) == E
    for change in ({"frames": 1}, {"frames": 0}, {"height": 0}, {"height": side + 1}, {"width": 0}, {"width": side + 1},
                   {"channels": 0}, {"channels": _cabi.LP_DETAIL_MAX_CHANNELS + 1}, {"reach": -1}, {"reach": _cabi.LP_TFILL_MAX_REACH + 1},
                   {"nearer": 2}, {"nearer": -1}, {"frame": -1}, {"frame": 5}, {"donor": 2}, {"donor": 4}, {"donor": 0},
                   {"frame": 0, "donor": -1}, {"frame": 4, "donor": 5}, {"org_src": None}, {"pos_src": None}):
        assert hip_lib.lp_tfill_carry(C.byref(_cabi.LpTfillCarryDesc(**{**good, **change})), None) == E, change
    for name in names:
        if name not in ("org_src", "pos_src"):                         # the donor's state: both null is "none"
            assert hip_lib.lp_tfill_carry(C.byref(_cabi.LpTfillCarryDesc(**{**good, name: None})), None) == E, name
    outs = ("org_dst", "pos_dst", "filled", "source", "remaining")
    for out in outs:                                                   # an output plane that is an input or another output
        for other in names:
            if other != out:
                assert hip_lib.lp_tfill_carry(C.byref(_cabi.LpTfillCarryDesc(**{**good, out: good[other]})), None) == E, (out, other)
    assert hip_lib.lp_tfill_carry(C.byref(_cabi.LpTfillCarryDesc(**{**good, "frames": 65536})), None) == U


def test_the_header_says_the_temporal_fill_words():
    header = open(os.path.join(ROOT, "include", "lanpaint_hip.h")).read()
    for word in ("LP_TFILL_MAX_REACH", "a tie stays with the past", "A tap with weight 0 is not read", "no FMA", "known = 1 - m",
                 "r = q - 16 i", "for every chunking"):
        assert word in header, word


# ---- the wrappers and the node ----------------------------------------------------------------------------------------------------------
def test_temporal_fill_refuses_cpu_tensors_and_bad_arguments():
    from lanpaint_amd import temporal_fill as tf
    images, mask = torch.zeros(4, 16, 16, 3), torch.zeros(4, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tf.temporal_fill(images, mask)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tf.temporal_fill(images.numpy(), mask)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tf.known_pyramids(mask, 4, 3)
    row = torch.zeros(2, _cabi.prop_pyramid_ws_bytes(1, 16, 16, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tf.step_fields(row, row, [(1, 0)], 16, 16, 3)
    planes = (torch.zeros(2, 2, 2, dtype=torch.int32), torch.zeros(16, 16, dtype=torch.uint8), torch.zeros(16, 16, dtype=torch.uint8), None,
              images, images.clone(), torch.zeros(4, 16, 16, dtype=torch.int32), mask.clone())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tf.carry(*planes, 1, 0)
    # the numbers are checked before the tensors are looked at
    for bad in (dict(levels=0), dict(levels=7), dict(levels=2.0), dict(search=0), dict(search=8), dict(smooth=-1), dict(smooth=65),
                dict(smooth=None), dict(reach=-1), dict(reach=65536), dict(reach=1.0), dict(reach=True)):
        with pytest.raises(ValueError):
            tf.temporal_fill(images, mask, **bad)
    for bad in (dict(levels=0), dict(levels=7), dict(frames=0), dict(frames=65536), dict(frame0=-1), dict(frame0=65532)):
        with pytest.raises(ValueError):
            tf.known_pyramids(mask, **{"frames": 4, "levels": 3, **bad})
    for bad in (dict(levels=0), dict(search=8), dict(smooth=65), dict(H=0), dict(W=_cabi.LP_VMASK_MAX_SIDE + 1)):
        with pytest.raises(ValueError):
            tf.step_fields(row, row, [(1, 0)], **{"H": 16, "W": 16, "levels": 3, **bad})
    for bad in (dict(reach=-1), dict(reach=65536)):
        with pytest.raises(ValueError):
            tf.carry(*planes, 1, 0, **bad)
    assert tf.WS_CAP_BYTES == 1 << 30 and tf.MAX_JOBS == 32 and tf.MAX_REACH == 65535 and tf.MAX_FRAMES == 65535


def test_node_protocol_and_own_mappings():
    from lanpaint_amd import temporal_fill_nodes
    node = temporal_fill_nodes.LanPaint_VideoTemporalFill
    assert temporal_fill_nodes.NODE_CLASS_MAPPINGS == {"LanPaint_VideoTemporalFill": node}
    assert list(temporal_fill_nodes.NODE_DISPLAY_NAME_MAPPINGS) == ["LanPaint_VideoTemporalFill"]
    types = node.INPUT_TYPES()
    req = types["required"]
    assert list(types) == ["required"] and list(req) == ["image", "mask", "levels", "search", "smooth", "reach"]
    assert req["image"][0] == "IMAGE" and req["mask"][0] == "MASK"
    assert req["levels"][0] == "INT" and req["levels"][1] == {**req["levels"][1], "default": 4, "min": 1, "max": 6}
    assert req["search"][0] == "INT" and req["search"][1] == {**req["search"][1], "default": 2, "min": 1, "max": 7}
    assert req["smooth"][0] == "INT" and req["smooth"][1] == {**req["smooth"][1], "default": 8, "min": 0, "max": 64}
    assert req["reach"][0] == "INT" and req["reach"][1] == {**req["reach"][1], "default": 0, "min": 0, "max": 65535}
    for name in req:
        assert len(req[name][1]["tooltip"]) > 20, name
    for word in ("other frames", "motion", "nearest frame", "mask fill", "encode", "Detailer", "remaining", "colour-matched"):
        assert word in node.DESCRIPTION, word
    assert node.RETURN_TYPES == ("IMAGE", "MASK", "MASK") and node.RETURN_NAMES == ("image", "remaining", "filled")
    assert node.FUNCTION == "fill" and callable(getattr(node, node.FUNCTION))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            node().fill(torch.zeros(3, 16, 16, 3), torch.zeros(3, 16, 16))
