"""The occlusion-aware video mask propagate, the parts that need no device: the restatement (tests/propagate_visible_ref.py) checked
on its own -- the properties the rule promises, as bits, and the quality conditions on a disc that passes behind a bar --, the two
C entries' argument checks (made before any HIP call), the node's protocol, and that the existing propagate modules are as they
were.  Layouts, constants and names against the header are tests/test_cabi_mirror.py's, for the whole C ABI."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi
from tests import propagate_ref as ref
from tests import propagate_visible_ref as vref
from tests.compare import _f32_bits as _bits, _iou
from tests.propagate_scenes import _texture, occluded_disc_clip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_OCCLUSION = 16


@functools.lru_cache(maxsize=None)
def _scored(name, occlusion):
    """Both rules on one clip: leak (mask pixels on the bar over the overlap frames), the mean IoU with disc-minus-bar over the
    frames after the disc has left the bar, and the hidden mass over the overlap frames, whole and on the bar."""
    kw = {"issue": dict(seed=0, F=16, H=64, W=96, radius=12, bar=(28, 44)),
          "wide": dict(seed=0, F=20, H=64, W=128, radius=20, bar=(46, 54))}[name]
    images, discs, on_bar = occluded_disc_clip(**kw)
    F = len(discs)
    overlap = [t for t in range(F) if (discs[t] & on_bar).any()]
    after = [t for t in range(F) if t > overlap[-1]]
    assert overlap and after and overlap[0] > 0
    key = discs[0].astype(np.float32)
    plain = ref.propagate_ref(images, key, 0, 3, 2, 8) >= 0.5
    mask, hidden = vref.propagate_visible_ref(images, key, 0, 3, 2, 8, occlusion)
    got, truth = mask >= 0.5, discs & ~on_bar
    return {"leak": sum(int((got[t] & on_bar).sum()) for t in overlap), "leak_plain": sum(int((plain[t] & on_bar).sum()) for t in overlap),
            "iou": float(np.mean([_iou(got[t], truth[t]) for t in after])), "iou_plain": float(np.mean([_iou(plain[t], truth[t]) for t in after])),
            "hidden": sum(float(hidden[t].sum()) for t in overlap), "hidden_on_bar": sum(float((hidden[t] * on_bar).sum()) for t in overlap)}


# ---- the restatement on its own: what follows from the rule -------------------------------------------------------------------------------
def test_equal_frames_return_the_binarised_key_mask_and_no_hidden_part():
    rng = np.random.default_rng(3)
    H, W = 23, 33
    soft = rng.random((H, W), dtype=np.float32)
    binar = np.repeat((soft >= np.float32(0.5)).astype(np.float32)[None], 4, axis=0)
    still = np.repeat(rng.random((1, H, W, 3), dtype=np.float32), 4, axis=0)
    for occlusion in (1, 16, 255):
        for key in (0, 2):
            mask, hidden = vref.propagate_visible_ref(still, soft, key, 3, 2, 8, occlusion)
            assert mask.dtype == hidden.dtype == np.float32
            assert (_bits(mask) == _bits(binar)).all() and (_bits(hidden) == 0).all(), (occlusion, key)
    one, hid = vref.propagate_visible_ref(still[:1], soft, 0, 3, 2, 8, 1)
    assert (_bits(one) == _bits(binar[:1])).all() and (_bits(hid) == 0).all()


@pytest.mark.parametrize("shift", [(2, -1), (-3, 5)], ids=str)
def test_a_whole_pixel_shift_away_from_the_border_is_never_taken_for_an_occluder(shift):
    F, H, W = 4, 96, 112
    big = (np.round(_texture(np.random.default_rng(79), 256, 256) * 255) / 255).astype(np.float32)
    images = np.stack([big[40 - shift[0] * t: 40 - shift[0] * t + H, 40 - shift[1] * t: 40 - shift[1] * t + W] for t in range(F)])
    mask = np.zeros((H, W), np.float32)
    mask[36:60, 40:70] = 1
    for occlusion in (1, 16):
        out, hidden = vref.propagate_visible_ref(images[..., None], mask, 0, 3, 2, 8, occlusion)
        for t in range(F):
            assert (_bits(out[t]) == _bits(np.roll(mask, (shift[0] * t, shift[1] * t), (0, 1)))).all(), (occlusion, t)
        assert (_bits(hidden) == 0).all()


def test_an_empty_mask_gives_zero_and_zero_and_occlusion_zero_is_the_plain_chain():
    rng = np.random.default_rng(5)
    H, W = 23, 33
    video = rng.random((4, H, W, 3), dtype=np.float32)
    for key in (0, 2, 3):
        mask, hidden = vref.propagate_visible_ref(video, np.zeros((H, W), np.float32), key, 3, 2, 8, 1)
        assert (_bits(mask) == 0).all() and (_bits(hidden) == 0).all()
    soft = rng.random((H, W), dtype=np.float32)
    mask, hidden = vref.propagate_visible_ref(video, soft, 1, 3, 2, 8, 0)
    assert (_bits(mask) == _bits(ref.propagate_ref(video, soft, 1, 3, 2, 8))).all() and (_bits(hidden) == 0).all()


def test_mask_plus_hidden_is_the_code_while_the_bits_equal_the_plain_chains():
    """Unrelated random frames: everything under the mask is 'occluded' at occlusion 1.  The first step starts from the key's bits
    in both chains, so mask + hidden = c / 256 of the plain chain there; at occlusion 255 nothing is ever flagged (a residual is at
    most 255 after the bias), the bits never part and the sum holds on every frame."""
    rng = np.random.default_rng(11)
    H, W = 40, 70
    video = rng.random((4, H, W, 1), dtype=np.float32)
    yy, xx = np.mgrid[:H, :W]
    disc = ((yy - 20) ** 2 + (xx - 30) ** 2 <= 15 ** 2).astype(np.float32)
    plain = ref.propagate_ref(video, disc, 1, 3, 2, 8)
    trace = {}
    mask, hidden = vref.propagate_visible_ref(video, disc, 1, 3, 2, 8, 1, trace)
    for t in (0, 2):                                                    # the first step of either chain
        assert (_bits(mask[t] + hidden[t]) == _bits(plain[t])).all(), t
        assert trace[t][2].any() and hidden[t].sum() > 0
        assert ((mask[t] * 256).astype(np.int64) == trace[t][3]).all() and (trace[t][3] <= trace[t][1]).all()
    mask, hidden = vref.propagate_visible_ref(video, disc, 1, 3, 2, 8, 255)
    assert (_bits(mask) == _bits(plain)).all() and (_bits(hidden) == 0).all()


def test_the_pieces_of_the_rule_one_at_a_time():
    H, W = 16, 24
    P = ref.key_positions(H, W)
    Yk = np.random.default_rng(1).integers(0, 256, (H, W)).astype(np.uint8)
    assert (vref.warped_key_luma(Yk, P) == Yk).all()
    full = np.ones((H, W), np.uint8)
    assert not vref.visible_flags(Yk, Yk, P, full, 1).any()
    # an exposure change of up to 32 grey levels is forgiven, in either direction; one of 34 leaves a residual of 2 per pixel
    Yk = np.full((H, W), 100, np.uint8)
    for shift, flagged in ((32, False), (-32, False), (34, True), (-34, True)):
        got = vref.visible_flags(np.full((H, W), 100 + shift, np.uint8), Yk, P, full, 1)
        assert got.all() == flagged and got.any() == flagged, shift
    assert not vref.visible_flags(np.full((H, W), 134, np.uint8), Yk, P, full, 2).any()          # R = 2 n is not above 2 n
    # the floor of the mean: d = -1 on 3 of 4 pixels gives mu = floor((2 * -192 + 256) / 512) = -1 in a full inner window ...
    Yt = Yk.copy()
    Yt[:, 1::4] += 1
    Yt -= 1
    assert (2 * -192 + 256) // 512 == -1
    got = vref.visible_flags(Yt, Yk, P, full, 1)                        # ... and R = n / 4: not above n
    assert not got.any()
    # fewer than 16 mask pixels in a window: no evidence, visible
    few = np.zeros((H, W), np.uint8)
    few[0:4, 4:8] = 1
    few[3, 7] = 0
    assert not vref.visible_flags(np.full((H, W), 255, np.uint8), np.zeros((H, W), np.uint8), P, few, 1).any()
    few[3, 7] = 1
    assert vref.visible_flags(np.full((H, W), 255, np.uint8), np.zeros((H, W), np.uint8), P, few, 1).tolist() == [[1, 1, 0], [0, 0, 0]]
    # the weight: 256 where all four blocks are visible, 0 where all are occluded, the advance's ramp between block centres
    flags = np.zeros((2, 3), np.int64)
    assert (vref.visibility_weight(flags, H, W) == 256).all() and (vref.visibility_weight(1 - flags, H, W) == 0).all()
    flags[:, 1] = 1
    w = vref.visibility_weight(flags, H, W)
    assert w[0, 0] == 256 and w[5, 3] == 256 and w[5, 11] == 16 and w[5, 12] == 16 and w[5, 7] == 9 * 16 == 144
    c = np.full((H, W), 256, np.int64)
    assert (vref.occlude(c, flags) == w).all() and (vref.occlude(np.zeros_like(c), flags) == 0).all()
    assert vref.VIS_MAX_BIAS == _cabi.LP_PROP_VIS_MAX_BIAS == 32


# ---- the quality conditions, on the restatement alone ---------------------------------------------------------------------------------------
def test_a_disc_that_passes_behind_a_bar():
    """64 x 96, 16 frames, levels 3: a disc of radius 12 moves 3 px per frame behind a static bar 16 px wide and out again; the
    truth per frame is the disc minus the bar.  At the default occlusion against propagate_ref on the same clip: (a) the leak is at
    most half of plain propagate's, (b) after the bar the IoU is not below plain propagate's, (c) the hidden part is not empty and
    lies on the bar for more than half of its mass.  Measured: leak 30 against 1382; hidden 3926, of it 3081 on the bar; IoU after
    the bar 0.000 for both rules -- the disc's visible rest (at most 8 px) is narrower than a block's window, so every block is
    flagged at once: this clip is a full occlusion at block granularity, which loses the subject under either rule."""
    s = _scored("issue", DEFAULT_OCCLUSION)
    print(s)
    assert 2 * s["leak"] <= s["leak_plain"]
    assert s["iou"] >= s["iou_plain"]
    assert s["hidden"] > 0 and 2 * s["hidden_on_bar"] > s["hidden"]


def test_the_mask_comes_back_when_part_of_the_subject_stays_in_view():
    """Point 4 of the rule where it can hold: a disc of radius 20 behind a bar 8 px wide always shows more than a window's width.
    With whole-pixel motion nothing but the bar and the noise raises a residual, so the test may be strict (occlusion 8): after the
    bar the mask is more than half way from nothing to the truth, where the plain rule has left the mask on the bar."""
    s = _scored("wide", 8)
    print(s)
    assert 2 * s["leak"] <= s["leak_plain"]
    assert s["iou"] > 0.5 > s["iou_plain"]


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_visible_and_occlude_reject_bad_arguments_without_a_device(hip_lib):
    C, E = ctypes, _cabi.LP_E_INVALID
    ptr = [C.c_void_p(256 << k) for k in range(5)]                      # never dereferenced: validation comes before any HIP call
    side = _cabi.LP_VMASK_MAX_SIDE
    assert hip_lib.lp_prop_visible(None, None) == E
    good = dict(height=40, width=70, occlusion=16, pos=ptr[0], tgt=ptr[1], key=ptr[2], mask=ptr[3], flags=ptr[4])
    for change in ({"height": 0}, {"height": side + 1}, {"width": 0}, {"width": side + 1}, {"occlusion": 0}, {"occlusion": -1},
                   {"occlusion": 256}, {"pos": None}, {"tgt": None}, {"key": None}, {"mask": None}, {"flags": None},
                   {"flags": ptr[0]}, {"flags": ptr[1]}, {"flags": ptr[2]}, {"flags": ptr[3]}):
        assert hip_lib.lp_prop_visible(C.byref(_cabi.LpPropVisibleDesc(**{**good, **change})), None) == E, change
    assert hip_lib.lp_prop_occlude(None, None) == E
    good = dict(height=40, width=70, levels=3, code=ptr[0], flags=ptr[1], out=ptr[2], hidden=ptr[3], mask_pyramid=ptr[4])
    for change in ({"height": 0}, {"height": side + 1}, {"width": 0}, {"width": side + 1}, {"levels": 0}, {"levels": 7},
                   {"code": None}, {"flags": None}, {"out": None}, {"hidden": None}, {"mask_pyramid": None},
                   {"out": ptr[0]}, {"out": ptr[1]}, {"hidden": ptr[0]}, {"hidden": ptr[1]}, {"hidden": ptr[2]},
                   {"mask_pyramid": ptr[0]}, {"mask_pyramid": ptr[1]}, {"mask_pyramid": ptr[2]}, {"mask_pyramid": ptr[3]}):
        assert hip_lib.lp_prop_occlude(C.byref(_cabi.LpPropOccludeDesc(**{**good, **change})), None) == E, change


def test_the_header_says_the_visible_words():
    header = open(os.path.join(ROOT, "include", "lanpaint_hip.h")).read()
    for word in ("LP_PROP_VIS_MAX_BIAS", "floor((2 D + n) / (2 n))", "R > occlusion * n", "c' = (c * w + 128) >> 8",
                 "hidden entirely", "Not handled: occlusion."):
        assert word in header, word


# ---- the wrapper and the node ---------------------------------------------------------------------------------------------------------
def test_propagate_visible_refuses_cpu_tensors_and_bad_arguments():
    from lanpaint_amd import propagate_visible as pv
    images, mask = torch.zeros(4, 16, 16, 3), torch.zeros(16, 16)
    u8 = torch.zeros(16, 16, dtype=torch.uint8)
    for call in (lambda: pv.propagate_masks_visible(images, mask), lambda: pv.propagate_masks_visible(images, mask, occlusion=0),
                 lambda: pv.visible_flags(torch.zeros(16, 16, 2, dtype=torch.int32), u8, u8, u8),
                 lambda: pv.occlude(torch.zeros(16, 16), torch.zeros(2, 2, dtype=torch.int32), 3)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for bad in (dict(occlusion=-1), dict(occlusion=256), dict(occlusion=16.0), dict(occlusion=True), dict(occlusion=None),
                dict(levels=0), dict(search=8), dict(smooth=65)):
        with pytest.raises(ValueError):
            pv.propagate_masks_visible(images, mask, **bad)
    with pytest.raises(ValueError):
        pv.visible_flags(torch.zeros(16, 16, 2, dtype=torch.int32), u8, u8, u8, 0)
    assert pv.DEFAULT_OCCLUSION == DEFAULT_OCCLUSION and pv.MAX_OCCLUSION == 255


def test_visible_node_protocol_and_the_existing_propagate_nodes_are_untouched():
    from lanpaint_amd import propagate_keys_nodes, propagate_nodes, propagate_visible_nodes
    node = propagate_visible_nodes.LanPaint_VideoMaskPropagateVisible
    assert propagate_visible_nodes.NODE_CLASS_MAPPINGS == {"LanPaint_VideoMaskPropagateVisible": node}
    assert propagate_visible_nodes.NODE_DISPLAY_NAME_MAPPINGS == {"LanPaint_VideoMaskPropagateVisible": "LanPaint Video Mask Propagate (Visible)"}
    assert propagate_nodes.NODE_CLASS_MAPPINGS == {"LanPaint_VideoMaskPropagate": propagate_nodes.LanPaint_VideoMaskPropagate}
    assert list(propagate_keys_nodes.NODE_CLASS_MAPPINGS) == ["LanPaint_VideoMaskPropagateKeys"]
    assert "occlusion is not handled" in propagate_nodes.LanPaint_VideoMaskPropagate.DESCRIPTION
    types = node.INPUT_TYPES()
    req = types["required"]
    assert list(types) == ["required"] and list(req) == ["image", "mask", "key_frame", "levels", "search", "smooth", "occlusion"]
    plain = propagate_nodes.LanPaint_VideoMaskPropagate.INPUT_TYPES()["required"]
    for name in ("key_frame", "levels", "search", "smooth"):
        assert req[name][0] == "INT" and {k: v for k, v in req[name][1].items() if k != "tooltip"} == \
            {k: v for k, v in plain[name][1].items() if k != "tooltip"}, name
    assert req["image"][0] == "IMAGE" and req["mask"][0] == "MASK"
    assert req["occlusion"][0] == "INT" and req["occlusion"][1] == {**req["occlusion"][1], "default": DEFAULT_OCCLUSION, "min": 0, "max": 255}
    for name in req:
        assert len(req[name][1]["tooltip"]) > 20, name
    assert node.RETURN_TYPES == ("MASK", "MASK") and node.RETURN_NAMES == ("mask", "hidden")
    assert node.FUNCTION == "propagate" and node.CATEGORY == "mask" and callable(getattr(node, node.FUNCTION))
    assert len(node.OUTPUT_TOOLTIPS) == 2 and "behind something" in node.OUTPUT_TOOLTIPS[1] and "through the occluder" in node.OUTPUT_TOOLTIPS[1]
    for word in ("one frame", "in front of the subject", "hidden", "stabilize", "mask refine", "Detailer", "One keyframe", "is lost"):
        assert word in node.DESCRIPTION, word
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            node().propagate(torch.zeros(4, 16, 16, 3), torch.zeros(16, 16), 0, 4, 2, 8, 16)
