"""The masked-area fill and the outpaint canvas, the parts that need no device: the restatement (tests/fill_ref.py) checked on its
own, plan_outpaint's arithmetic, the pad's mask rule on an example written out by hand, the three C entries' argument checks (made
before any HIP call), lp_fill_ws_bytes against its Python mirror, the nodes' protocol and the no-fallback errors.  Layouts,
constants and names against the header are tests/test_cabi_mirror.py's, for the whole C ABI."""
import ctypes
import dataclasses
import os

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, fill
from tests import fill_ref

WS_CASES = [(1, 1, 1, 1), (1, 1, 2, 1), (2, 17, 33, 3), (3, 32, 32, 4), (1, 2049, 1, 5), (81, 720, 1280, 3), (65535, 32768, 32768, 64)]
REF_SHAPES = [(1, 1), (1, 7), (7, 1), (63, 65), (64, 64), (129, 65), (130, 200)]


def _image(H, W, C=3, seed=0):
    rng = np.random.default_rng([H, W, C, seed])
    return (np.float32(0.05) + np.float32(0.95) * rng.random((1, H, W, C), dtype=np.float32)).astype(np.float32)


def _speckle(H, W, seed=1):
    return (np.random.default_rng([H, W, seed]).random((1, H, W)) < 0.3).astype(np.float32)


# ---- the restatement on its own -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", REF_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_restatement_keeps_known_pixels_and_fills_from_them(hw):
    H, W = hw
    img, mask = _image(H, W), _speckle(H, W)
    mask[0, H // 2, W // 2] = np.nan                                # a NaN is not > 0.5: known
    out = fill_ref.fill_ref(img, mask)
    known = ~(mask > 0.5)
    assert out.dtype == np.float32 and out.shape == img.shape
    assert known[0, H // 2, W // 2] and (out.view(np.uint32)[known] == img.view(np.uint32)[known]).all()
    assert out.min() >= img[known].min() and out.max() <= img[known].max()
    # the same rule in fp64: the rule's own rounding stays within 1e-6 on inputs in [0.05, 1)
    assert np.abs(out.astype(np.float64) - fill_ref.fill_ref(img, mask, np.float64)).max() <= 1e-6
    # what the image holds under the mask does not matter
    poisoned = np.where((mask > 0.5)[..., None], np.float32(np.nan), img).astype(np.float32)
    assert (fill_ref.fill_ref(poisoned, mask).view(np.uint32) == out.view(np.uint32)).all()
    # no known pixel: unchanged; one known pixel: constant
    assert (fill_ref.fill_ref(img, np.ones((1, H, W), np.float32)).view(np.uint32) == img.view(np.uint32)).all()
    one = np.ones((1, H, W), dtype=np.float32)
    one[0, H - 1, 0] = 0.0
    assert (fill_ref.fill_ref(img, one) == img[:, H - 1:, :1]).all()


def test_the_restatement_on_an_example_worked_by_hand():
    # 2 x 3, one channel; pixels (0, 1) and (1, 1) are masked.  Level 1 is 1 x 2: means {(1 + 5) / 2, (3 + 7) / 2} = {3, 5}, level 2
    # their mean 4.  Push: level 1 is known everywhere.  Row taps of both rows clamp to coarse row 0; column 1 is odd:
    # i0 = 0, weights (0.75, 0.25): 0.75 * 3 + 0.25 * 5 = 3.5
    img = np.array([[[1.0], [100.0], [3.0]], [[5.0], [-100.0], [7.0]]], dtype=np.float32)[None]
    mask = np.array([[0, 1, 0], [0, 1, 0]], dtype=np.float32)[None]
    assert fill_ref.levels(2, 3) == [(2, 3), (1, 2), (1, 1)] and len(fill_ref.levels(720, 1280)) == 12
    assert len(fill_ref.levels(32768, 1)) == 16
    assert fill_ref.fill_ref(img, mask)[0, :, :, 0].tolist() == [[1.0, 3.5, 3.0], [5.0, 3.5, 7.0]]


def test_the_pad_rule_on_an_example_worked_by_hand():
    # 3 x 4 image, 1 column on the left, 2 on the right, 2 rows at the bottom, overlap 1: a 5 x 7 canvas.  The band covers the
    # outside, the original's first and last column (left and right are padded) and its last row (bottom is); not its first row.
    img = np.arange(1, 13, dtype=np.float32).reshape(1, 3, 4, 1)
    soft = np.array([[0.0, 0.25, np.nan, 0.0], [0.0, 0.0, 0.75, 0.0], [0.5, 0.0, 0.0, 0.0]], dtype=np.float32)[None]
    canvas, mask = fill_ref.pad_ref(img, soft, 1, 0, 2, 2, 1)
    assert canvas[0, :, :, 0].tolist() == [[0, 1, 2, 3, 4, 0, 0], [0, 5, 6, 7, 8, 0, 0], [0, 9, 10, 11, 12, 0, 0],
                                           [0] * 7, [0] * 7]
    assert mask[0].tolist() == [[1, 1, 0.25, 0, 1, 1, 1], [1, 1, 0, 0.75, 1, 1, 1], [1] * 7, [1] * 7, [1] * 7]
    _, plain = fill_ref.pad_ref(img, None, 0, 2, 0, 0, 0)
    assert plain.shape == (1, 5, 4) and plain[0].tolist() == [[1] * 4, [1] * 4, [0] * 4, [0] * 4, [0] * 4]


# ---- the plan -------------------------------------------------------------------------------------------------------------------------
def test_plan_outpaint_snaps_each_axis_by_its_branch():
    P = fill.OutpaintPlan
    # both sides: 30 + 52 + 11 = 93 -> e = 3: 1 low, 2 high.  high only: 0 + 40 + 5 = 45 -> e = 3, all of it at the bottom
    assert fill.plan_outpaint(40, 52, 30, 0, 11, 5, 6, 8) == P(31, 0, 13, 8, 6, 48, 96)
    # low only on both axes: 7 + 50 = 57 -> e = 7;  3 + 20 = 23 -> e = 1
    assert fill.plan_outpaint(20, 50, 7, 3, 0, 0, 0, 8) == P(14, 4, 0, 0, 0, 24, 64)
    # an unpadded axis is left alone even when it is no multiple: width 50 stays
    assert fill.plan_outpaint(20, 50, 0, 0, 0, 4, 0, 8) == P(0, 0, 0, 4, 0, 24, 50)
    # already a multiple: e = 0;  M = 1: nothing moves
    assert fill.plan_outpaint(480, 480, 200, 0, 200, 0, 16, 8) == P(200, 0, 200, 0, 16, 480, 880)
    assert fill.plan_outpaint(33, 35, 1, 2, 3, 4, 5, 1) == P(1, 2, 3, 4, 5, 39, 39)
    # both sides, odd remainder: 1 + 10 + 1 = 12 -> e = 4: 2 and 2;  1 + 9 + 1 = 11 -> e = 5: 2 low, 3 high
    assert fill.plan_outpaint(9, 10, 1, 1, 1, 1, 0, 8) == P(3, 3, 3, 4, 0, 16, 16)
    assert dataclasses.is_dataclass(P) and P.__dataclass_params__.frozen
    # the overlap may take all but one pixel
    assert fill.plan_outpaint(9, 10, 1, 0, 1, 0, 4, 1).width == 12


def test_plan_outpaint_refusals():
    good = dict(H=40, W=52, left=8, top=0, right=8, bottom=0, overlap=4, multiple_of=8)
    fill.plan_outpaint(**good)
    for change in ({"left": 0, "right": 0}, {"left": -8}, {"top": -1}, {"right": -1}, {"bottom": -2}, {"overlap": -1},
                   {"multiple_of": 0}, {"multiple_of": -8}, {"overlap": 26}, {"overlap": 52, "right": 0},
                   {"top": 8, "bottom": 8, "overlap": 20}, {"left": _cabi.LP_DETAIL_MAX_SIDE}, {"bottom": _cabi.LP_DETAIL_MAX_SIDE - 39},
                   {"left": 8.0}, {"overlap": True}, {"H": 0}):
        with pytest.raises(ValueError):
            fill.plan_outpaint(**{**good, **change})
    assert fill.plan_outpaint(**{**good, "overlap": 25}).overlap == 25            # 2 x 25 < 52
    assert fill.plan_outpaint(**{**good, "overlap": 51, "right": 0}).overlap == 51
    assert fill.plan_outpaint(**{**good, "left": 0, "right": 0, "bottom": _cabi.LP_DETAIL_MAX_SIDE - 40}).height == 32768


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_mask_fill_rejects_bad_arguments_without_a_device(hip_lib):
    C, E, U, A = ctypes, _cabi.LP_E_INVALID, _cabi.LP_E_UNSUPPORTED, _cabi.LP_E_ALIGN
    p, q = C.c_void_p(256), C.c_void_p(512)                # never dereferenced: validation comes before any HIP call
    F = _cabi.LpFillDesc
    assert hip_lib.lp_mask_fill(None, None) == E
    ws = _cabi.fill_ws_bytes(2, 40, 150, 3)
    good = dict(batch=2, height=40, width=150, channels=3, mask_batch=1, reserved0=0, image=p, mask=p, out=q, ws=p, ws_bytes=ws)
    for change in ({"batch": 0}, {"batch": -1}, {"height": 0}, {"height": _cabi.LP_DETAIL_MAX_SIDE + 1}, {"width": 0},
                   {"width": _cabi.LP_DETAIL_MAX_SIDE + 1}, {"channels": 0}, {"channels": _cabi.LP_DETAIL_MAX_CHANNELS + 1},
                   {"mask_batch": 0}, {"mask_batch": 3}, {"image": None}, {"mask": None}, {"out": None}, {"ws": None},
                   {"ws_bytes": ws - 1}, {"ws_bytes": 0}, {"out": p}):
        assert hip_lib.lp_mask_fill(C.byref(F(**{**good, **change})), None) == E, change
    assert hip_lib.lp_mask_fill(C.byref(F(**{**good, "ws": 260})), None) == A
    big = {**good, "batch": 65536, "ws_bytes": 1 << 40}
    assert hip_lib.lp_mask_fill(C.byref(F(**big)), None) == U
    assert hip_lib.lp_mask_fill(C.byref(F(**{**big, "mask_batch": 65536})), None) == U
    # the limits themselves are inside: the next refusal is the short workspace
    edge = {**good, "channels": 64, "height": _cabi.LP_DETAIL_MAX_SIDE, "ws_bytes": 1}
    assert hip_lib.lp_mask_fill(C.byref(F(**edge)), None) == E
    assert hip_lib.lp_mask_fill(C.byref(F(**{**edge, "ws": 264})), None) == A


def test_fill_ws_bytes_equals_its_mirror_and_refuses_bad_arguments(hip_lib):
    for case in WS_CASES:
        assert hip_lib.lp_fill_ws_bytes(*case) == _cabi.fill_ws_bytes(*case), case
    assert _cabi.fill_ws_bytes(1, 1, 1, 1) == 16                                   # one level: nothing to keep, never 0 bytes
    assert _cabi.fill_ws_bytes(1, 1, 2, 1) == 16                                   # 1 pixel: 4 + 1 bytes
    levels = _cabi.fill_levels(720, 1280)
    assert len(levels) == 12 and levels[1] == (360, 640) and levels[-1] == (1, 1) and levels == fill_ref.levels(720, 1280)
    pix = sum(h * w for h, w in levels[1:])
    assert _cabi.fill_ws_bytes(81, 720, 1280, 3) == (81 * pix * 13 + 15) // 16 * 16
    E, U = _cabi.LP_E_INVALID, _cabi.LP_E_UNSUPPORTED
    for bad in ((0, 8, 8, 3), (-1, 8, 8, 3), (1, 0, 8, 3), (1, 8, 0, 3), (1, 32769, 8, 3), (1, 8, 32769, 3), (1, 8, 8, 0), (1, 8, 8, 65)):
        assert hip_lib.lp_fill_ws_bytes(*bad) == E, bad
    assert hip_lib.lp_fill_ws_bytes(65536, 8, 8, 3) == U


def test_outpaint_pad_rejects_bad_arguments_without_a_device(hip_lib):
    C, E, U = ctypes, _cabi.LP_E_INVALID, _cabi.LP_E_UNSUPPORTED
    p = C.c_void_p(256)
    O = _cabi.LpOutpaintDesc
    assert hip_lib.lp_outpaint_pad(None, None) == E
    good = dict(batch=2, height=40, width=150, channels=3, mask_batch=1, left=8, top=0, right=0, bottom=16, overlap=4, reserved0=0,
                image=p, mask=p, image_out=p, mask_out=p)
    M = _cabi.LP_DETAIL_MAX_SIDE
    for change in ({"batch": 0}, {"height": 0}, {"height": M + 1}, {"width": -3}, {"width": M + 1}, {"channels": 0}, {"channels": 65},
                   {"mask_batch": 3}, {"mask_batch": -1}, {"image": None}, {"mask": None}, {"image_out": None}, {"mask_out": None},
                   {"left": -1}, {"top": -1}, {"right": -1}, {"bottom": -1}, {"overlap": -1}, {"left": 0, "bottom": 0},
                   {"left": M - 149}, {"bottom": M - 39}, {"top": 1 << 30, "bottom": 1 << 30}):
        assert hip_lib.lp_outpaint_pad(C.byref(O(**{**good, **change})), None) == E, change
    assert hip_lib.lp_outpaint_pad(C.byref(O(**{**good, "batch": 65536})), None) == U
    assert hip_lib.lp_outpaint_pad(C.byref(O(**{**good, "batch": 65536, "mask_batch": 0, "mask": None})), None) == U


def test_the_fill_kernels_are_a_source_of_the_build():
    from lanpaint_amd import build
    assert "fill_kernel.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "fill_kernel.hip"))


# ---- the wrappers and the nodes -------------------------------------------------------------------------------------------------------
def test_fill_functions_refuse_cpu_tensors():
    img, mask = torch.zeros(2, 16, 16, 3), torch.zeros(2, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fill.fill_masked(img, mask)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fill.outpaint_pad(img, None, left=8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fill.outpaint_pad(img, mask, left=8, fill=False)


def test_fill_nodes_protocol_and_own_mappings():
    from lanpaint_amd import fill_nodes
    pad, mf = fill_nodes.LanPaint_OutpaintPad, fill_nodes.LanPaint_MaskFill
    assert fill_nodes.NODE_CLASS_MAPPINGS == {"LanPaint_OutpaintPad": pad, "LanPaint_MaskFill": mf}
    assert fill_nodes.NODE_DISPLAY_NAME_MAPPINGS == {"LanPaint_OutpaintPad": "LanPaint Outpaint Pad",
                                                     "LanPaint_MaskFill": "LanPaint Mask Fill"}
    types = pad.INPUT_TYPES()
    req = types["required"]
    assert list(req) == ["image", "left", "top", "right", "bottom", "overlap", "multiple_of", "fill"]
    assert req["image"][0] == "IMAGE" and list(types["optional"]) == ["mask"] and types["optional"]["mask"][0] == "MASK"
    for side in ("left", "top", "right", "bottom"):
        assert req[side][0] == "INT" and req[side][1] == {**req[side][1], "default": 0, "min": 0, "max": 8192, "step": 8}
    assert req["overlap"][0] == "INT" and req["overlap"][1] == {**req["overlap"][1], "default": 16, "min": 0, "max": 512}
    assert req["multiple_of"][0] == "INT" and req["multiple_of"][1] == {**req["multiple_of"][1], "default": 8, "min": 1, "max": 128}
    assert req["fill"][0] == "BOOLEAN" and req["fill"][1]["default"] is True
    assert pad.RETURN_TYPES == ("IMAGE", "MASK") and pad.RETURN_NAMES == ("image", "mask")
    assert pad.FUNCTION == "pad" and pad.CATEGORY == "image" and callable(getattr(pad, pad.FUNCTION))
    req = mf.INPUT_TYPES()["required"]
    assert list(req) == ["image", "mask"] and req["image"][0] == "IMAGE" and req["mask"][0] == "MASK"
    assert mf.RETURN_TYPES == ("IMAGE",) and mf.FUNCTION == "fill" and mf.CATEGORY == "image" and callable(getattr(mf, mf.FUNCTION))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            mf().fill(torch.zeros(2, 16, 16, 3), torch.zeros(2, 16, 16))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pad().pad(torch.zeros(2, 16, 16, 3), left=8)
