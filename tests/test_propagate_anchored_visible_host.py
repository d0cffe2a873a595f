"""The anchored occlusion-aware video mask propagate, the parts that need no device: the restatement
(tests/propagate_anchored_visible_ref.py) checked on its own -- that the rule does what it is for, on clips with sub-pixel motion
and an occluder, and the properties it promises, as bits --, the C entry's argument checks (made before any HIP call), the nodes'
protocol, and that the existing node modules are as they were.  Layouts, constants and names against the header are
tests/test_cabi_mirror.py's, for the whole C ABI."""
import ctypes
import os

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi
from tests import propagate_anchored_ref as aref
from tests import propagate_anchored_visible_ref as avref
from tests import propagate_ref as ref
from tests import propagate_visible_ref as vref
from tests.anchor_clips import subpixel_clip
from tests.compare import _f32_bits as _bits
from tests.propagate_scenes import (QUALITY_DEFAULTS as DEFAULTS, QUALITY_OCCLUSION as OCCLUSION, anchored_quality_case as quality_case,
                                    assert_the_anchored_quality_lines as assert_the_quality_lines, whole_subject_iou)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement on its own ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_the_new_form_holds_the_subject_behind_an_occluder_where_each_existing_form_loses_it(name):
    _, truth, new, anchored, visible = quality_case(name)
    assert_the_quality_lines(name, truth, new, anchored, visible)
    assert (_bits(new[0][0]) == _bits(truth[0].astype(np.float32))).all() and not new[1][0].any()      # the key frame


def test_with_no_occluder_the_visible_form_collapses_and_the_new_form_is_the_anchored_form():
    """Measured: the visible restatement's last-frame IoU is 0.000; no block is gated and no flag fires in the new form."""
    _, truth, new, anchored, visible = quality_case("N")
    last = whole_subject_iou(*visible, truth)[0]
    print("visible, last frame", last)
    assert last <= 0.10
    assert (_bits(new[0]) == _bits(anchored)).all() and (_bits(new[1]) == 0).all()


@pytest.mark.parametrize("vx", [0, 1])
def test_a_still_clip_and_a_whole_pixel_shift_give_the_plain_bits_and_a_zero_hidden(vx):
    images, truth = subpixel_clip(9, 40, 56, vy=0, vx=vx, noise=0)
    key = truth[0].astype(np.float32)
    plain = ref.propagate_ref(images, key, *DEFAULTS)
    for anchor in (1, 2, 7):
        trace = {}
        got, hidden = avref.propagate_anchored_visible_ref(images, key, *DEFAULTS, anchor, OCCLUSION, trace)
        assert sorted(trace) == list(range(1, 9))
        for t in trace:
            assert not trace[t][2].any() and not trace[t][3].any() and not trace[t][6].any(), (anchor, t)   # gated, e, flags
        assert (_bits(got) == _bits(plain)).all() and (_bits(hidden) == 0).all(), anchor


def test_empty_one_frame_and_the_three_off_forms():
    images, truth = subpixel_clip(4, 23, 33)
    H, W = 23, 33
    for key in (0, 2, 3):
        got, hidden = avref.propagate_anchored_visible_ref(images, np.zeros((H, W), np.float32), key, 3, 2, 8, 2, 16)
        assert (_bits(got) == 0).all() and (_bits(hidden) == 0).all()
    soft = np.random.default_rng(5).random((H, W), dtype=np.float32)
    one, hidden = avref.propagate_anchored_visible_ref(images[:1], soft, 0, 3, 2, 8, 2, 16)
    assert (_bits(one) == _bits(ref.binarise(soft).astype(np.float32)[None])).all() and (_bits(hidden) == 0).all()
    zeros = np.zeros((4, H, W), np.uint32)
    for anchor, occlusion, want in ((0, 16, vref.propagate_visible_ref(images, soft, 1, 3, 2, 8, 16)),
                                    (2, 0, (aref.propagate_anchored_ref(images, soft, 1, 3, 2, 8, 2), zeros)),
                                    (0, 0, (ref.propagate_ref(images, soft, 1, 3, 2, 8), zeros))):
        got = avref.propagate_anchored_visible_ref(images, soft, 1, 3, 2, 8, anchor, occlusion)
        assert (_bits(got[0]) == _bits(want[0])).all() and (_bits(got[1]) == _bits(want[1])).all(), (anchor, occlusion)


def test_the_gate_is_the_visible_statistic_at_the_alignment_the_match_found():
    rng = np.random.default_rng(7)
    H, W = 24, 40
    Yk = rng.integers(0, 256, (H, W)).astype(np.uint8)
    P = ref.key_positions(H, W)
    full = np.ones((H, W), np.uint8)
    Yt = np.roll(Yk, (1, -2), (0, 1))                                   # the frame lies (1, -2) from where the chain has it
    want_vec, want_valid = aref.anchor_field(P, Yt, Yk, full, 2, 0)
    vec, valid, gated = avref.gated_anchor_field(P, Yt, Yk, full, 2, 0, 16)
    inner = (slice(1, -1), slice(1, -1))
    assert not gated[inner].any() and valid[inner].all() and (vec[inner] == (16, -32)).all()     # drift is no occluder
    assert vref.visible_flags(Yt, Yk, P, full, 16)[inner].all()         # the test at the carried positions takes it for one
    Yt = Yt.copy()
    Yt[:, 24:] = rng.integers(0, 256, (H, 16))                          # something else in front of the right-hand blocks
    vec, valid, gated = avref.gated_anchor_field(P, Yt, Yk, full, 2, 0, 16)
    want_vec, want_valid = aref.anchor_field(P, Yt, Yk, full, 2, 0)
    assert gated[:, 4:].all() and not gated[1:-1, 1:2].any()
    assert (valid == (want_valid & (gated == 0))).all() and (vec == np.where(gated[..., None] != 0, 0, want_vec)).all()
    few = np.zeros((H, W), np.uint8)
    few[0:4, 4:8] = 1
    few[3, 7] = 0                                                       # 15 mask pixels: no block is live
    vec, valid, gated = avref.gated_anchor_field(P, Yt, Yk, few, 2, 0, 1)
    assert not valid.any() and not vec.any() and not gated.any()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_anchor_match_gated_rejects_bad_arguments_without_a_device(hip_lib):
    C, E = ctypes, _cabi.LP_E_INVALID
    ptr = [C.c_void_p(256 << k) for k in range(7)]                      # never dereferenced: validation comes before any HIP call
    side = _cabi.LP_VMASK_MAX_SIDE
    assert hip_lib.lp_prop_anchor_match_gated(None, None) == E
    good = dict(height=40, width=70, anchor=2, smooth=8, occlusion=16, reserved0=0, pos=ptr[0], tgt=ptr[1], key=ptr[2], mask=ptr[3],
                vec=ptr[4], valid=ptr[5], gated=ptr[6])
    changes = [{"height": 0}, {"height": side + 1}, {"width": 0}, {"width": side + 1}, {"anchor": 0}, {"anchor": -1}, {"anchor": 8},
               {"smooth": -1}, {"smooth": 65}, {"occlusion": 0}, {"occlusion": -1}, {"occlusion": 256}, {"reserved0": 1},
               {"reserved0": -1}]
    changes += [{name: None} for name in ("pos", "tgt", "key", "mask", "vec", "valid", "gated")]
    changes += [{out: ptr[k]} for out in ("vec", "valid", "gated") for k in range(4)]           # an output on an input
    changes += [{"valid": ptr[4]}, {"gated": ptr[4]}, {"gated": ptr[5]}]                         # an output on another output
    for change in changes:
        assert hip_lib.lp_prop_anchor_match_gated(C.byref(_cabi.LpPropAnchorGatedDesc(**{**good, **change})), None) == E, change


def test_the_header_and_the_documents_say_the_gated_words():
    header = open(os.path.join(ROOT, "include", "lanpaint_hip.h")).read()
    for word in ("Video mask propagate, anchored and occlusion-aware", "the block is gated iff R > occlusion * n",
                 "valid = live and not gated", "a subject hidden entirely", "several keys"):
        assert word in header, word
    for doc in ("README.md", "DESIGN.md", "CHANGES.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "LanPaint_VideoMaskPropagateAnchoredVisible" in text, doc
    from lanpaint_amd import propagate_anchored, propagate_visible
    for module in (propagate_anchored, propagate_visible):              # the two forms' documents point here
        assert "propagate_anchored_visible.py" in module.__doc__


# ---- the wrapper and the nodes --------------------------------------------------------------------------------------------------------
def test_propagate_anchored_visible_refuses_cpu_tensors_and_bad_arguments():
    from lanpaint_amd import propagate_anchored_visible as pav
    images, mask = torch.zeros(4, 16, 16, 3), torch.zeros(16, 16)
    u8 = torch.zeros(16, 16, dtype=torch.uint8)
    pos = torch.zeros(16, 16, 2, dtype=torch.int32)
    for call in (lambda: pav.propagate_masks_anchored_visible(images, mask),
                 lambda: pav.propagate_masks_anchored_visible(images, mask, anchor=0),
                 lambda: pav.propagate_masks_anchored_visible(images, mask, occlusion=0),
                 lambda: pav.propagate_masks_anchored_visible(images, mask, anchor=0, occlusion=0),
                 lambda: pav.gated_anchor_field(pos, u8, u8, u8)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for bad in (dict(anchor=-1), dict(anchor=8), dict(anchor=2.0), dict(anchor=True), dict(anchor=None), dict(occlusion=-1),
                dict(occlusion=256), dict(occlusion=16.0), dict(levels=0), dict(search=8), dict(smooth=65)):
        with pytest.raises(ValueError):
            pav.propagate_masks_anchored_visible(images, mask, **bad)
    for bad in (dict(anchor=0), dict(anchor=8), dict(smooth=65), dict(occlusion=0), dict(occlusion=256)):
        with pytest.raises(ValueError):
            pav.gated_anchor_field(pos, u8, u8, u8, **bad)
    assert pav.DEFAULT_ANCHOR == 2 and pav.MAX_ANCHOR == 7 and pav.DEFAULT_OCCLUSION == 16 and pav.MAX_OCCLUSION == 255
    from lanpaint_amd import propagate, propagate_anchored, propagate_visible
    for module in (pav, propagate_anchored, propagate_visible):        # one step and one chain loop, propagate's, behind every form
        assert module.Step is propagate.Step
        assert not [n for n, v in vars(module).items() if isinstance(v, type) and v.__module__ == module.__name__], module
        assert not hasattr(module, "chain") and "def chain" not in open(module.__file__).read(), module
    for word in ("a subject hidden entirely", "what leaves the picture", "occlusion edges finer than a block", "several keys",
                 "a subject whose look changes away from the key"):
        assert word in pav.__doc__, word


# every other node module's mappings, as they were before this module came
OTHER_NODE_NAMES = {
    "propagate_nodes": ["LanPaint_VideoMaskPropagate"],
    "propagate_keys_nodes": ["LanPaint_VideoMaskPropagateKeys"],
    "propagate_visible_nodes": ["LanPaint_VideoMaskPropagateVisible"],
    "propagate_keys_visible_nodes": ["LanPaint_VideoMaskPropagateKeysVisible"],
    "propagate_anchored_nodes": ["LanPaint_VideoMaskPropagateAnchored", "LanPaint_VideoMaskPropagateAnchoredShots"],
}


def test_anchored_visible_node_protocol_and_the_existing_node_modules_are_untouched():
    import importlib

    from lanpaint_amd import propagate_anchored_visible_nodes as mine
    from lanpaint_amd import propagate_nodes, shots_nodes
    node = mine.LanPaint_VideoMaskPropagateAnchoredVisible
    per_shot = mine.LanPaint_VideoMaskPropagateAnchoredVisibleShots
    assert mine.NODE_CLASS_MAPPINGS == {"LanPaint_VideoMaskPropagateAnchoredVisible": node,
                                        "LanPaint_VideoMaskPropagateAnchoredVisibleShots": per_shot}
    assert mine.NODE_DISPLAY_NAME_MAPPINGS == {
        "LanPaint_VideoMaskPropagateAnchoredVisible": "LanPaint Video Mask Propagate (Anchored, Visible)",
        "LanPaint_VideoMaskPropagateAnchoredVisibleShots": "LanPaint Video Mask Propagate (Anchored, Visible, Shots)"}
    for module, names in OTHER_NODE_NAMES.items():
        assert list(importlib.import_module(f"lanpaint_amd.{module}").NODE_CLASS_MAPPINGS) == names, module
    assert len(shots_nodes.NODE_CLASS_MAPPINGS) == 7
    types = node.INPUT_TYPES()
    req = types["required"]
    assert list(types) == ["required"]
    assert list(req) == ["image", "mask", "key_frame", "levels", "search", "smooth", "anchor", "occlusion"]
    plain = propagate_nodes.LanPaint_VideoMaskPropagate.INPUT_TYPES()["required"]
    for name in ("key_frame", "levels", "search", "smooth"):
        assert req[name][0] == "INT" and {k: v for k, v in req[name][1].items() if k != "tooltip"} == \
            {k: v for k, v in plain[name][1].items() if k != "tooltip"}, name
    assert req["image"][0] == plain["image"][0] == "IMAGE" and req["mask"][0] == plain["mask"][0] == "MASK"
    assert req["anchor"][0] == "INT" and req["anchor"][1] == {**req["anchor"][1], "default": 2, "min": 0, "max": 7}
    assert req["occlusion"][0] == "INT" and req["occlusion"][1] == {**req["occlusion"][1], "default": 16, "min": 0, "max": 255}
    for name in req:
        assert len(req[name][1]["tooltip"]) > 20, name
    assert node.RETURN_TYPES == ("MASK", "MASK") and node.RETURN_NAMES == ("mask", "hidden") and len(node.OUTPUT_TOOLTIPS) == 2
    assert node.FUNCTION == "propagate" and node.CATEGORY == "mask" and callable(getattr(node, node.FUNCTION))
    for word in ("one frame", "key frame again", "long clip", "in front of the subject", "`hidden`", "stabilize", "mask refine", "Detailer",
                 "hidden entirely", "leaves the picture", "finer than a block", "several keys", "look changes"):
        assert word in node.DESCRIPTION, word
    assert issubclass(per_shot, node) and per_shot.__mro__[1] is shots_nodes._PerShot
    assert per_shot.INPUT_TYPES()["required"] == req and list(per_shot.INPUT_TYPES()["optional"]) == ["shots"]
    assert per_shot.propagate is not node.propagate and "shot" in per_shot.DESCRIPTION
    if not torch.cuda.is_available():
        for cls in (node, per_shot):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                cls().propagate(torch.zeros(4, 16, 16, 3), torch.zeros(16, 16), 0, 4, 2, 8, 2, 16)
    for bad in ((-1, 16), (8, 16), (2, -1), (2, 256)):                  # outside 0..7 and 0..255 raises, with or without a device
        with pytest.raises(ValueError):
            node().propagate(torch.zeros(4, 16, 16, 3), torch.zeros(16, 16), 0, 4, 2, 8, *bad)
