"""The anchored video mask propagate, the parts that need no device: the restatement (tests/propagate_anchored_ref.py) checked on its
own -- that the rule does what it is for, on a clip with sub-pixel motion, and the properties it promises, as bits --, the C
entry's argument checks (made before any HIP call), the nodes' protocol, and that the existing propagate nodes are as they were.
Layouts, constants and names against the header are tests/test_cabi_mirror.py's, for the whole C ABI."""
import ctypes
import os

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi
from tests import propagate_anchored_ref as aref
from tests import propagate_ref as ref
from tests.anchor_clips import subpixel_clip
from tests.compare import _f32_bits as _bits
from tests.propagate_scenes import assert_the_two_drift_iou_lines as assert_the_two_iou_lines, drift_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement on its own ---------------------------------------------------------------------------------------------------------------
def test_the_plain_chain_drifts_on_subpixel_motion_and_the_anchored_chain_does_not():
    _, truth, plain, anchored = drift_case()
    assert_the_two_iou_lines(truth, plain, anchored)
    assert (_bits(anchored[0]) == _bits(truth[0].astype(np.float32))).all()        # the key frame returns its binarised mask


@pytest.mark.parametrize("vx", [0, 1])
def test_a_still_clip_and_a_whole_pixel_shift_give_a_zero_correction_and_the_plain_bits(vx):
    images, truth = subpixel_clip(9, 40, 56, vy=0, vx=vx, noise=0)
    key = truth[0].astype(np.float32)
    for anchor in (1, 2, 7):
        trace = {}
        got = aref.propagate_anchored_ref(images, key, 0, 4, 2, 8, anchor, trace)
        assert sorted(trace) == list(range(1, 9))
        for t in trace:
            assert not trace[t][2].any(), (anchor, t)                              # e = 0 on every frame
        assert (_bits(got) == _bits(ref.propagate_ref(images, key, 0, 4, 2, 8))).all(), anchor


def test_empty_full_one_frame_and_anchor_zero():
    images, truth = subpixel_clip(4, 23, 33)
    H, W = 23, 33
    for key in (0, 2, 3):
        assert (_bits(aref.propagate_anchored_ref(images, np.zeros((H, W), np.float32), key, 3, 2, 8, 2)) == 0).all()
        full = aref.propagate_anchored_ref(images, np.ones((H, W), np.float32), key, 3, 2, 8, 2)
        assert (_bits(full) == _bits(np.ones((4, H, W), np.float32))).all()
    soft = np.random.default_rng(5).random((H, W), dtype=np.float32)
    one = aref.propagate_anchored_ref(images[:1], soft, 0, 3, 2, 8, 2)
    assert (_bits(one) == _bits(ref.binarise(soft).astype(np.float32)[None])).all()
    off = aref.propagate_anchored_ref(images, soft, 1, 3, 2, 8, 0)
    assert (_bits(off) == _bits(ref.propagate_ref(images, soft, 1, 3, 2, 8))).all()


def test_the_correction_field_is_the_level_0_match_of_the_warped_key_luma():
    rng = np.random.default_rng(7)
    H, W = 24, 40
    Yk = rng.integers(0, 256, (H, W)).astype(np.uint8)
    P = ref.key_positions(H, W)
    assert (aref.warped_key_luma(Yk, P) == Yk).all()
    full = np.ones((H, W), np.uint8)
    vec, valid = aref.anchor_field(P, Yk, Yk, full, 2, 8)
    assert valid.all() and not vec.any()
    Yt = np.roll(Yk, (1, -2), (0, 1))                                               # the frame lies (1, -2) from where the chain has it
    vec, valid = aref.anchor_field(P, Yt, Yk, full, 2, 0)
    assert (vec[1:-1, 1:-1] == (16, -32)).all()
    few = np.zeros((H, W), np.uint8)
    few[0:4, 4:8] = 1
    few[3, 7] = 0                                                                   # 15 mask pixels: no block is valid
    vec, valid = aref.anchor_field(P, Yt, Yk, few, 2, 0)
    assert not valid.any() and not vec.any()                                        # an invalid block holds 0


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_anchor_match_rejects_bad_arguments_without_a_device(hip_lib):
    C, E = ctypes, _cabi.LP_E_INVALID
    ptr = [C.c_void_p(256 << k) for k in range(6)]                      # never dereferenced: validation comes before any HIP call
    side = _cabi.LP_VMASK_MAX_SIDE
    assert hip_lib.lp_prop_anchor_match(None, None) == E
    good = dict(height=40, width=70, anchor=2, smooth=8, pos=ptr[0], tgt=ptr[1], key=ptr[2], mask=ptr[3], vec=ptr[4], valid=ptr[5])
    for change in ({"height": 0}, {"height": side + 1}, {"width": 0}, {"width": side + 1}, {"anchor": 0}, {"anchor": -1},
                   {"anchor": 8}, {"smooth": -1}, {"smooth": 65}, {"pos": None}, {"tgt": None}, {"key": None}, {"mask": None},
                   {"vec": None}, {"valid": None}, {"vec": ptr[0]}, {"vec": ptr[1]}, {"vec": ptr[2]}, {"vec": ptr[3]},
                   {"valid": ptr[0]}, {"valid": ptr[1]}, {"valid": ptr[2]}, {"valid": ptr[3]}, {"valid": ptr[4]}, {"vec": ptr[5]}):
        assert hip_lib.lp_prop_anchor_match(C.byref(_cabi.LpPropAnchorDesc(**{**good, **change})), None) == E, change


def test_the_header_and_the_documents_say_the_anchor_words():
    header = open(os.path.join(ROOT, "include", "lanpaint_hip.h")).read()
    for word in ("Video mask propagate, anchored", "An invalid block holds 0", "predictor p = 0", "anchor = 0 is the caller's",
                 "re-anchoring every n-th frame only"):
        assert word in header, word
    for doc in ("README.md", "DESIGN.md", "CHANGES.md", "INTEGRATION.md"):
        assert "LanPaint_VideoMaskPropagateAnchored" in open(os.path.join(ROOT, doc)).read(), doc


# ---- the wrapper and the nodes --------------------------------------------------------------------------------------------------------
def test_propagate_anchored_refuses_cpu_tensors_and_bad_arguments():
    from lanpaint_amd import propagate_anchored as pa
    images, mask = torch.zeros(4, 16, 16, 3), torch.zeros(16, 16)
    u8 = torch.zeros(16, 16, dtype=torch.uint8)
    for call in (lambda: pa.propagate_masks_anchored(images, mask), lambda: pa.propagate_masks_anchored(images, mask, anchor=0),
                 lambda: pa.anchor_field(torch.zeros(16, 16, 2, dtype=torch.int32), u8, u8, u8)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for bad in (dict(anchor=-1), dict(anchor=8), dict(anchor=2.0), dict(anchor=True), dict(anchor=None), dict(levels=0), dict(search=8),
                dict(smooth=65)):
        with pytest.raises(ValueError):
            pa.propagate_masks_anchored(images, mask, **bad)
    for bad in (dict(anchor=0), dict(anchor=8), dict(smooth=65)):
        with pytest.raises(ValueError):
            pa.anchor_field(torch.zeros(16, 16, 2, dtype=torch.int32), u8, u8, u8, **bad)
    assert pa.DEFAULT_ANCHOR == 2 and pa.MAX_ANCHOR == 7


def test_anchored_node_protocol_and_the_existing_propagate_nodes_are_untouched():
    from lanpaint_amd import propagate_anchored_nodes, propagate_nodes, shots_nodes
    node = propagate_anchored_nodes.LanPaint_VideoMaskPropagateAnchored
    per_shot = propagate_anchored_nodes.LanPaint_VideoMaskPropagateAnchoredShots
    assert propagate_anchored_nodes.NODE_CLASS_MAPPINGS == {"LanPaint_VideoMaskPropagateAnchored": node,
                                                            "LanPaint_VideoMaskPropagateAnchoredShots": per_shot}
    assert propagate_anchored_nodes.NODE_DISPLAY_NAME_MAPPINGS == {
        "LanPaint_VideoMaskPropagateAnchored": "LanPaint Video Mask Propagate (Anchored)",
        "LanPaint_VideoMaskPropagateAnchoredShots": "LanPaint Video Mask Propagate (Anchored, Shots)"}
    assert propagate_nodes.NODE_CLASS_MAPPINGS == {"LanPaint_VideoMaskPropagate": propagate_nodes.LanPaint_VideoMaskPropagate}
    assert len(shots_nodes.NODE_CLASS_MAPPINGS) == 7
    types = node.INPUT_TYPES()
    req = types["required"]
    assert list(types) == ["required"] and list(req) == ["image", "mask", "key_frame", "levels", "search", "smooth", "anchor"]
    plain = propagate_nodes.LanPaint_VideoMaskPropagate.INPUT_TYPES()["required"]
    for name in ("key_frame", "levels", "search", "smooth"):
        assert req[name][0] == "INT" and {k: v for k, v in req[name][1].items() if k != "tooltip"} == \
            {k: v for k, v in plain[name][1].items() if k != "tooltip"}, name
    assert req["image"][0] == "IMAGE" and req["mask"][0] == "MASK"
    assert req["anchor"][0] == "INT" and req["anchor"][1] == {**req["anchor"][1], "default": 2, "min": 0, "max": 7}
    for name in req:
        assert len(req[name][1]["tooltip"]) > 20, name
    assert node.RETURN_TYPES == ("MASK",) and node.RETURN_NAMES == ("mask",)
    assert node.FUNCTION == "propagate" and node.CATEGORY == "mask" and callable(getattr(node, node.FUNCTION))
    for word in ("one frame", "key frame again", "long clip", "stabilize", "mask refine", "Detailer", "One keyframe", "drifts as before"):
        assert word in node.DESCRIPTION, word
    assert issubclass(per_shot, node) and per_shot.__mro__[1] is shots_nodes._PerShot
    assert per_shot.INPUT_TYPES()["required"] == req and list(per_shot.INPUT_TYPES()["optional"]) == ["shots"]
    assert per_shot.propagate is not node.propagate and "shot" in per_shot.DESCRIPTION
    if not torch.cuda.is_available():
        for cls in (node, per_shot):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                cls().propagate(torch.zeros(4, 16, 16, 3), torch.zeros(16, 16), 0, 4, 2, 8, 2)
    for bad in (-1, 8):                                                  # anchor outside 0..7 raises, with or without a device
        with pytest.raises(ValueError):
            node().propagate(torch.zeros(4, 16, 16, 3), torch.zeros(16, 16), 0, 4, 2, 8, bad)
