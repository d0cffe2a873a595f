"""The mask refine, the parts that need no device: the restatement (tests/refine_ref.py) checked on its own -- the properties the
rule promises, as bits, the edge snap it exists for, grow_mask's rule against a brute-force disc --, the two C entries' argument
checks (made before any HIP call), lp_refine_ws_bytes against its Python mirror, the node's protocol and the no-fallback errors.
Layouts, constants and names against the header are tests/test_cabi_mirror.py's, for the whole C ABI."""
import ctypes
import os

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, refine
from tests import refine_ref as ref
from tests.compare import _raw_bits as _bits

SHAPES = [(1, 1), (1, 7), (7, 1), (5, 9), (33, 65), (40, 70)]
RADII = (1, 3, 8, 64)


def _guide(H, W, C=3, seed=0):
    return np.random.default_rng([H, W, C, seed]).random((H, W, C), dtype=np.float32)


def _soft(H, W, seed=1):
    return np.random.default_rng([H, W, seed]).random((H, W), dtype=np.float32)


def _near(on, r):
    """[H, W] bool: within Chebyshev distance r of a True pixel."""
    return ref.box_int(on.astype(np.int64), r) > 0


def _box_mean_integral(a, r):
    """The mean over the cut window through an integral image in fp64: an independent statement of the box blur."""
    H, W = a.shape
    ii = np.zeros((H + 1, W + 1), dtype=np.float64)
    ii[1:, 1:] = np.cumsum(np.cumsum(a.astype(np.float64), axis=0), axis=1)
    out = np.empty((H, W), dtype=np.float64)
    for y in range(H):
        ya, yb = max(y - r, 0), min(y + r, H - 1) + 1
        for x in range(W):
            xa, xb = max(x - r, 0), min(x + r, W - 1) + 1
            out[y, x] = (ii[yb, xb] - ii[ya, xb] - ii[yb, xa] + ii[ya, xa]) / ((yb - ya) * (xb - xa))
    return out


# ---- the restatement on its own -------------------------------------------------------------------------------------------------------
def test_codes_rule():
    v = np.array([-1.0, -0.0, 0.0, 1e-30, 0.002, 0.0019, 0.3, 1.0, 1.5, np.inf,
                  -np.inf, np.nan], dtype=np.float32)
    assert ref.codes(v).tolist() == [0, 0, 0, 0, 1, 0, 77, 255, 255, 255, 0, 0]
    k = np.arange(256)
    assert (ref.codes((k / 255.0).astype(np.float32)) == k).all()


@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_restatement_keeps_what_the_rule_promises(hw):
    H, W = hw
    for C in (1, 3, 4):
        g = _guide(H, W, C)
        for r in RADII:
            for eps in (1e-6, 1e-3, 1.0):
                zero = ref.refine_image(g, np.zeros((H, W), np.float32), r, eps)
                one = ref.refine_image(g, np.ones((H, W), np.float32), r, eps)
                assert zero.dtype == np.float32 and zero.shape == (H, W)
                assert (_bits(zero) == 0).all(), (C, r, eps)
                assert (_bits(one) == _bits(np.ones((H, W), np.float32))).all(), (C, r, eps)
    soft = ref.refine_image(_guide(H, W), _soft(H, W), 3, 1e-3)
    assert (soft >= 0).all() and (soft <= 1).all()
    assert (_bits(soft) == _bits(ref.refine_image(_guide(H, W), _soft(H, W), 3, 1e-3))).all()
    # channels beyond the third are not read
    g4 = _guide(H, W, 5)
    assert (_bits(ref.refine_image(g4, _soft(H, W), 3, 1e-3)) == _bits(ref.refine_image(g4[..., :3], _soft(H, W), 3, 1e-3))).all()
    with pytest.raises(ValueError):
        ref.refine_image(_guide(H, W, 2), _soft(H, W), 3, 1e-3)


@pytest.mark.parametrize("r", [1, 3, 8])
@pytest.mark.parametrize("C", [1, 3])
def test_the_restatement_reaches_2r_and_no_further(r, C):
    H, W = 60, 75
    g = _guide(H, W, C, 3)
    for eps in (1e-6, 1e-3):
        spots = np.zeros((H, W), np.float32)
        spots[30, 40], spots[0, 0], spots[59, 10:13] = 1.0, 0.3, 2.0
        spots[10, 70], spots[45, 60] = -1.0, np.nan                  # code 0: they reach nowhere
        spots[20, 20] = 0.4 / 255                                    # rounds to code 0
        out = ref.refine_image(g, spots, r, eps)
        far = ~_near(ref.codes(spots) > 0, 2 * r)
        assert far.any() and (_bits(out)[far] == 0).all() and (out != 0).any()
        holes = (1.0 - np.nan_to_num(np.clip(spots, 0, 1))).astype(np.float32)
        out = ref.refine_image(g, holes, r, eps)
        far = ~_near(ref.codes(holes) < 255, 2 * r)
        assert far.any() and (_bits(out)[far] == _bits(np.float32(1.0))).all() and (out != 1).any()
    # the reach is attained: a single pixel under a constant guide spreads exactly 2r
    point = np.zeros((H, W), np.float32)
    point[30, 40] = 1.0
    out = ref.refine_image(np.full((H, W, C), 0.5, np.float32), point, r, 1e-3)
    assert ((out != 0) == _near(point > 0, 2 * r)).all()


@pytest.mark.parametrize("hw", [(1, 7), (5, 9), (33, 65)], ids=lambda s: "x".join(map(str, s)))
def test_a_constant_guide_gives_the_double_box_blur(hw):
    H, W = hw
    mask = _soft(H, W, 4)
    P = ref.codes(mask)
    for r in (1, 3, 8):
        for C, level in ((3, 0.5), (1, 0.0), (3, 1.0)):
            out = ref.refine_image(np.full((H, W, C), level, np.float32), mask, r, 1e-3)
            # a = 0 exactly, b = the box mean of P rounded to fp32; out = the box mean of b / 255.  The integral image sums in
            # another order: each of the two means carries a few fp64 roundings, the fp32 rounding of b 2^-24 relative
            b = _box_mean_integral(P, r).astype(np.float32)
            want = _box_mean_integral(b, r) / 255.0
            assert np.abs(out.astype(np.float64) - want).max() <= 2.0 ** -23, (r, C, level)
            # and bit for bit against the header's own order
            n = ref.count(H, W, r).astype(np.float64)
            b2 = (ref.box_int(P, r).astype(np.float64) / n).astype(np.float32)
            assert (_bits(b2) == _bits(b)).all()
            exact = np.clip(ref.box_f64(b2.astype(np.float64), r) / n / 255.0, 0, 1).astype(np.float32)
            assert (_bits(out) == _bits(exact)).all(), (r, C, level)


def test_the_filter_snaps_a_rough_edge_onto_the_images():
    H, W, r, eps = 96, 128, 8, 1e-3
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W]
    true = (xx + 0.3 * yy) < 70
    guide = np.where(true[..., None], [0.8, 0.3, 0.2], [0.2, 0.5, 0.7]).astype(np.float32)
    guide = guide + rng.normal(0, 0.02, (H, W, 3)).astype(np.float32)
    rough = ((xx + 0.3 * yy + 3 * np.sin(yy / 3.0)) < 70).astype(np.float32)
    out = ref.refine_image(guide, rough, r, eps)
    rough_wrong = int(((rough > 0.5) != true).sum())
    refined_wrong = int(((out > 0.5) != true).sum())
    print("rough wrong", rough_wrong, "refined wrong", refined_wrong)
    assert rough_wrong == 181
    assert refined_wrong <= rough_wrong // 10, (rough_wrong, refined_wrong)


# ---- grow_mask's rule -----------------------------------------------------------------------------------------------------------------
def _disc_grow(mask, grow):
    """grow_mask by its meaning: the union of discs of radius `grow` around foreground pixels; shrinking is growing the
    background by a disc and taking what is left.  Pixel by pixel, no distance transform."""
    fg = np.asarray(mask, dtype=np.float32) >= np.float32(0.5)
    H, W = fg.shape
    src = fg if grow > 0 else ~fg
    R = abs(grow)
    hit = np.zeros((H, W), dtype=bool)
    for y, x in zip(*np.nonzero(src)):
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                if dy * dy + dx * dx <= R * R and 0 <= y + dy < H and 0 <= x + dx < W:
                    hit[y + dy, x + dx] = True
    return (hit if grow > 0 else fg & ~hit).astype(np.float32)


@pytest.mark.parametrize("grow", [-5, -2, -1, 1, 2, 5, 40])
def test_grow_rule_is_a_euclidean_disc(grow):
    rng = np.random.default_rng(abs(grow) * 2 + (grow < 0))
    H, W = 17, 23
    blobs = np.zeros((H, W), np.float32)
    blobs[3:12, 4:15] = 1.0
    blobs[6, 8] = 0.0
    blobs[14, 20] = 0.5
    blobs[0, 22] = 0.49999
    masks = [blobs, (rng.random((H, W)) < 0.1).astype(np.float32), (rng.random((H, W)) < 0.9).astype(np.float32)]
    if abs(grow) > 5:
        masks = masks[:1]
    for m in masks:
        assert (ref.grow_ref(m, grow) == _disc_grow(m, grow)).all()
    for m in (np.zeros((H, W), np.float32), np.ones((H, W), np.float32)):
        assert (ref.grow_ref(m, grow) == m).all()
    soft = rng.random((H, W), dtype=np.float32)
    assert ref.grow_ref(soft, 0) is soft


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_mask_refine_rejects_bad_arguments_without_a_device(hip_lib):
    C, E, U, A = ctypes, _cabi.LP_E_INVALID, _cabi.LP_E_UNSUPPORTED, _cabi.LP_E_ALIGN
    p, q, r = C.c_void_p(256), C.c_void_p(512), C.c_void_p(768)     # never dereferenced: validation comes before any HIP call
    M = _cabi.LpRefineDesc
    assert hip_lib.lp_mask_refine(None, None) == E
    ws = _cabi.refine_ws_bytes(2, 40, 150, 3, 8)
    good = dict(batch=2, height=40, width=150, channels=3, mask_batch=1, radius=8, eps=1e-3, guide=p, mask=r, out=q, ws=p,
                ws_bytes=ws)
    for change in ({"batch": 0}, {"batch": -1}, {"height": 0}, {"height": _cabi.LP_DETAIL_MAX_SIDE + 1}, {"width": 0},
                   {"width": _cabi.LP_DETAIL_MAX_SIDE + 1}, {"channels": 0}, {"channels": 2}, {"channels": -3},
                   {"channels": _cabi.LP_DETAIL_MAX_CHANNELS + 1}, {"mask_batch": 0}, {"mask_batch": 3}, {"radius": 0},
                   {"radius": -1}, {"radius": _cabi.LP_REFINE_MAX_RADIUS + 1}, {"eps": 0.0}, {"eps": 0.99e-6}, {"eps": 1.0000001},
                   {"eps": -1e-3}, {"eps": float("nan")}, {"eps": float("inf")}, {"guide": None}, {"mask": None}, {"out": None},
                   {"ws": None}, {"ws_bytes": ws - 1}, {"ws_bytes": 0}, {"out": p}, {"out": r}):
        assert hip_lib.lp_mask_refine(C.byref(M(**{**good, **change})), None) == E, change
    assert hip_lib.lp_mask_refine(C.byref(M(**{**good, "ws": 260})), None) == A
    big = {**good, "batch": 65536, "ws_bytes": 1 << 40}
    assert hip_lib.lp_mask_refine(C.byref(M(**big)), None) == U
    assert hip_lib.lp_mask_refine(C.byref(M(**{**big, "mask_batch": 65536})), None) == U
    # the limits themselves are inside: the next refusal is the short workspace
    for inside in ({"channels": 1}, {"channels": 64}, {"radius": 1}, {"radius": 64}, {"eps": 1e-6}, {"eps": 1.0},
                   {"height": _cabi.LP_DETAIL_MAX_SIDE}, {"mask_batch": 2}):
        edge = {**good, **inside, "ws_bytes": 1}
        assert hip_lib.lp_mask_refine(C.byref(M(**edge)), None) == E, inside
        assert hip_lib.lp_mask_refine(C.byref(M(**{**edge, "ws": 264})), None) == A, inside


def test_refine_ws_bytes_equals_its_mirror(hip_lib):
    for case in ((1, 1, 1, 1, 1), (2, 17, 33, 3, 8), (3, 32, 32, 4, 64), (81, 720, 1280, 3, 8), (65535, 32768, 32768, 64, 64),
                 (1, 7, 1, 1, 3)):
        assert hip_lib.lp_refine_ws_bytes(*case) == _cabi.refine_ws_bytes(*case) == case[0] * case[1] * case[2] * 16, case
    assert _cabi.refine_ws_bytes(1, 1, 1, 3, 1) == 16
    assert 81 * 720 * 1280 * 16 > refine.WS_CAP_BYTES == 1 << 30    # the 81-frame clip runs in more than one chunk
    E, U = _cabi.LP_E_INVALID, _cabi.LP_E_UNSUPPORTED
    for bad in ((0, 8, 8, 3, 8), (-1, 8, 8, 3, 8), (1, 0, 8, 3, 8), (1, 8, 0, 3, 8), (1, 32769, 8, 3, 8), (1, 8, 32769, 3, 8),
                (1, 8, 8, 0, 8), (1, 8, 8, 2, 8), (1, 8, 8, 65, 8), (1, 8, 8, 3, 0), (1, 8, 8, 3, 65), (1, 8, 8, 3, -1)):
        assert hip_lib.lp_refine_ws_bytes(*bad) == E, bad
    assert hip_lib.lp_refine_ws_bytes(65536, 8, 8, 3, 8) == U


def test_the_refine_kernels_are_a_source_of_the_build():
    from lanpaint_amd import build
    assert "refine_kernel.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "refine_kernel.hip"))


# ---- the wrapper and the node ---------------------------------------------------------------------------------------------------------
def test_refine_refuses_cpu_tensors():
    img, mask = torch.zeros(2, 16, 16, 3), torch.zeros(2, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        refine.refine_mask(img, mask)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        refine.refine_mask(img, mask, radius=0, grow=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        refine.grow_mask(mask, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        refine.grow_mask(mask, 0)


def test_refine_node_protocol_and_own_mappings():
    from lanpaint_amd import refine_nodes
    node = refine_nodes.LanPaint_MaskRefine
    assert refine_nodes.NODE_CLASS_MAPPINGS == {"LanPaint_MaskRefine": node}
    assert refine_nodes.NODE_DISPLAY_NAME_MAPPINGS == {"LanPaint_MaskRefine": "LanPaint Mask Refine"}
    types = node.INPUT_TYPES()
    req = types["required"]
    assert list(types) == ["required"] and list(req) == ["image", "mask", "grow", "radius", "eps"]
    assert req["image"][0] == "IMAGE" and req["mask"][0] == "MASK"
    assert req["grow"][0] == "INT" and req["grow"][1] == {**req["grow"][1], "default": 0, "min": -256, "max": 256}
    assert req["radius"][0] == "INT" and req["radius"][1] == {**req["radius"][1], "default": 8, "min": 0, "max": 64}
    assert req["eps"][0] == "FLOAT" and req["eps"][1] == {**req["eps"][1], "default": 1e-3, "min": 1e-6, "max": 1.0}
    for name in req:
        assert len(req[name][1]["tooltip"]) > 20, name
    assert "encode" in node.DESCRIPTION and "video mask editor" in node.DESCRIPTION
    assert node.RETURN_TYPES == ("MASK",) and node.FUNCTION == "refine" and node.CATEGORY == "mask"
    assert callable(getattr(node, node.FUNCTION))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            node().refine(torch.zeros(2, 16, 16, 3), torch.zeros(2, 16, 16), 0, 8, 1e-3)
