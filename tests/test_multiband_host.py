"""The multiband blend, the parts that need no device: the restatement (tests/multiband_ref.py) checked on its own -- the properties
the rule promises, as bits, and REDUCE / EXPAND against an independent statement of Burt-Adelson --, the two C entries' argument
checks (made before any HIP call), lp_multiband_ws_bytes against its Python mirror and the closed form, the node's protocol and
the no-fallback errors.  Layouts, constants and names against the header are tests/test_cabi_mirror.py's, for the whole C ABI."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lanpaint_amd import _cabi, multiband
from tests import multiband_ref as ref
from tests.compare import _raw_bits as _bits

LEVELS = (0, 1, 2, 3, 5, 12)
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (63, 65), (64, 64), (130, 200), (300, 300)]
WS_CASES = [(1, 1, 1, 1, 5), (1, 1, 2, 1, 1), (1, 1, 2, 1, 0), (2, 17, 33, 3, 2), (3, 32, 32, 4, 16), (1, 2049, 1, 5, 12),
            (81, 720, 1280, 3, 5), (65535, 32768, 32768, 64, 16), (4, 300, 300, 3, 0)]


def _image(H, W, C=3, seed=0, B=1):
    rng = np.random.default_rng([H, W, C, seed])
    return (np.float32(0.05) + np.float32(0.95) * rng.random((B, H, W, C), dtype=np.float32)).astype(np.float32)


def _soft(H, W, seed=1):
    return np.random.default_rng([H, W, seed]).random((1, H, W), dtype=np.float32)


def _near(mask, r):
    """[Bm, H, W] bool: within Chebyshev distance r of a pixel with W_0 > 0 (a box sum over an integral image)."""
    on = ref.weight0(mask) > 0
    Bm, H, W = on.shape
    ii = np.zeros((Bm, H + 1, W + 1), dtype=np.int64)
    ii[:, 1:, 1:] = on.cumsum(1).cumsum(2)
    y0, y1 = np.clip(np.arange(H) - r, 0, H), np.clip(np.arange(H) + r + 1, 0, H)
    x0, x1 = np.clip(np.arange(W) - r, 0, W), np.clip(np.arange(W) + r + 1, 0, W)
    box = ii[:, y1][:, :, x1] - ii[:, y0][:, :, x1] - ii[:, y1][:, :, x0] + ii[:, y0][:, :, x0]
    return box > 0


# ---- the restatement on its own -------------------------------------------------------------------------------------------------------
def test_level_sizes_and_reach():
    assert ref.level_sizes(1, 1, 5) == [(1, 1)]
    assert ref.level_sizes(3, 5, 12) == [(3, 5), (2, 3), (1, 2), (1, 1)]
    assert ref.level_sizes(720, 1280, 5) == [(720, 1280), (360, 640), (180, 320), (90, 160), (45, 80), (23, 40)]
    assert ref.level_sizes(720, 1280, 0) == [(720, 1280)] and len(ref.level_sizes(32768, 1, 16)) == 16
    assert [ref.reach(n) for n in range(1, 6)] == [4, 12, 28, 60, 124]
    for hw in SHAPES:
        for levels in LEVELS:
            assert _cabi.multiband_levels(*hw, levels) == ref.level_sizes(*hw, levels)


@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_restatement_keeps_what_the_rule_promises(hw):
    H, W = hw
    a, b = _image(H, W, 3, 0), _image(H, W, 3, 1)
    soft = _soft(H, W)
    soft[0, H // 2, W // 2] = np.nan
    full = len(ref.level_sizes(H, W, 99)) - 1
    for levels in LEVELS:
        out = ref.blend_ref(a, b, soft, levels)
        assert out.dtype == np.float32 and out.shape == a.shape
        # image1 == image2: image1 as bits whatever the mask;  an all-zero mask: image1 as bits
        assert (_bits(ref.blend_ref(a, a, soft, levels)) == _bits(a)).all()
        assert (_bits(ref.blend_ref(a, b, np.zeros((1, H, W), np.float32), levels)) == _bits(a)).all()
        # an all-one mask: image2 within rounding
        one = ref.blend_ref(a, b, np.ones((1, H, W), np.float32), levels)
        assert np.abs(one - b).max() <= 5e-7, float(np.abs(one - b).max())
        # levels beyond the halvings change nothing
        if levels >= full:
            assert (_bits(out) == _bits(ref.blend_ref(a, b, soft, full))).all()
        # the same rule in fp64.  A level adds at most 16 fp32 roundings to a value of R (two 3-tap expansions of R and of D, the
        # difference, the product, the sum) and as many through REDUCE, each of a magnitude below 2: 2^-23 apiece
        n = min(levels, full)
        assert np.abs(out.astype(np.float64) - ref.blend_ref(a, b, soft, levels, np.float64)).max() <= 32 * (n + 1) * 2.0 ** -23
    w0 = ref.weight0(soft)[..., None]
    assert (_bits(ref.blend_ref(a, b, soft, 0)) == _bits(a + w0 * (b - a))).all() and w0[0, H // 2, W // 2, 0] == 0


@pytest.mark.parametrize("levels", LEVELS)
def test_the_restatement_reaches_no_further_than_the_bound(levels):
    H, W = 300, 300
    a, b = _image(H, W, 2, 2), _image(H, W, 2, 3)
    n = len(ref.level_sizes(H, W, levels)) - 1
    point = np.zeros((1, H, W), np.float32)
    point[0, 150, 149] = 1.0
    spots = np.zeros((1, H, W), np.float32)
    spots[0, 0, 0], spots[0, 299, 130], spots[0, 77:80, 200:203] = 0.25, 2.0, 0.5
    spots[0, 10, 290], spots[0, 200, 50] = -1.0, np.nan              # W_0 = 0: they reach nowhere
    for mask in (point, spots):
        out = ref.blend_ref(a, b, mask, levels)
        far = ~_near(mask, ref.reach(n))
        assert (_bits(out)[far] == _bits(a)[far]).all()
        assert (out != a).any()
        if n <= 5:
            assert far.any()


def test_weight0_rule():
    m = np.array([[-1.0, -0.0, 0.0, 1e-30, 0.3, 1.0, 1.5, np.inf, -np.inf, np.nan]], dtype=np.float32)[None]
    assert ref.weight0(m)[0, 0].tolist() == [0, 0, 0, np.float32(1e-30), np.float32(0.3), 1, 1, 1, 0, 0]


@pytest.mark.parametrize("hw", [(1, 1), (1, 7), (2, 2), (3, 5), (64, 64), (63, 65), (130, 201)], ids=lambda s: "x".join(map(str, s)))
def test_reduce_is_the_burt_adelson_kernel_at_stride_two(hw):
    H, W = hw
    x = np.random.default_rng([H, W, 5]).random((2, H, W, 3))
    k = torch.tensor(ref.K5, dtype=torch.float64)
    kern = torch.outer(k, k)[None, None]
    t = torch.from_numpy(x).permute(0, 3, 1, 2).reshape(6, 1, H, W)
    padded = F.pad(t, (2, 2, 2, 2), mode="replicate")
    want = F.conv2d(padded, kern, stride=2).reshape(2, 3, (H + 1) // 2, (W + 1) // 2).permute(0, 2, 3, 1).numpy()
    got = ref.reduce(x)
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12
    assert sum(ref.K5) == 1.0


def test_expand_keeps_a_constant_and_a_linear_ramp():
    for h, w in ((1, 1), (2, 3), (7, 8), (33, 64)):
        c = np.full((1, (h + 1) // 2, (w + 1) // 2, 2), 0.7, dtype=np.float64)
        assert np.abs(ref.expand(c, h, w) - 0.7).max() <= 1e-15
        c32 = np.full((1, (h + 1) // 2, (w + 1) // 2, 2), 0.75, dtype=np.float32)
        assert (ref.expand(c32, h, w) == np.float32(0.75)).all()
    # coarse sample p sits at fine index 2 p: a ramp in coarse coordinates comes back as the ramp at half the slope
    h, w = 41, 60
    yy, xx = np.meshgrid(np.arange((h + 1) // 2, dtype=np.float64), np.arange((w + 1) // 2, dtype=np.float64), indexing="ij")
    c = (3.0 * yy - 2.0 * xx + 1.0)[None, :, :, None]
    fy, fx = np.meshgrid(np.arange(h) / 2.0, np.arange(w) / 2.0, indexing="ij")
    want = 3.0 * fy - 2.0 * fx + 1.0
    got = ref.expand(c, h, w)[0, :, :, 0]
    assert np.abs(got - want)[2:-2, 2:-2].max() <= 1e-12


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_multiband_blend_rejects_bad_arguments_without_a_device(hip_lib):
    C, E, U, A = ctypes, _cabi.LP_E_INVALID, _cabi.LP_E_UNSUPPORTED, _cabi.LP_E_ALIGN
    p, q, r = C.c_void_p(256), C.c_void_p(512), C.c_void_p(768)     # never dereferenced: validation comes before any HIP call
    M = _cabi.LpMultibandDesc
    assert hip_lib.lp_multiband_blend(None, None) == E
    ws = _cabi.multiband_ws_bytes(2, 40, 150, 3, 5)
    good = dict(batch=2, height=40, width=150, channels=3, mask_batch=1, levels=5, image1=p, image2=r, mask=p, out=q, ws=p,
                ws_bytes=ws)
    for change in ({"batch": 0}, {"batch": -1}, {"height": 0}, {"height": _cabi.LP_DETAIL_MAX_SIDE + 1}, {"width": 0},
                   {"width": _cabi.LP_DETAIL_MAX_SIDE + 1}, {"channels": 0}, {"channels": _cabi.LP_DETAIL_MAX_CHANNELS + 1},
                   {"mask_batch": 0}, {"mask_batch": 3}, {"levels": -1}, {"image1": None}, {"image2": None}, {"mask": None},
                   {"out": None}, {"ws": None}, {"ws_bytes": ws - 1}, {"ws_bytes": 0}, {"out": p}, {"out": r}):
        assert hip_lib.lp_multiband_blend(C.byref(M(**{**good, **change})), None) == E, change
    assert hip_lib.lp_multiband_blend(C.byref(M(**{**good, "ws": 260})), None) == A
    big = {**good, "batch": 65536, "ws_bytes": 1 << 40}
    assert hip_lib.lp_multiband_blend(C.byref(M(**big)), None) == U
    assert hip_lib.lp_multiband_blend(C.byref(M(**{**big, "mask_batch": 65536})), None) == U
    # the limits themselves are inside: the next refusal is the short workspace
    edge = {**good, "channels": 64, "height": _cabi.LP_DETAIL_MAX_SIDE, "levels": 1 << 30, "ws_bytes": 1}
    assert hip_lib.lp_multiband_blend(C.byref(M(**edge)), None) == E
    assert hip_lib.lp_multiband_blend(C.byref(M(**{**edge, "ws": 264})), None) == A


def test_multiband_ws_bytes_equals_its_mirror_and_the_closed_form(hip_lib):
    for case in WS_CASES:
        assert hip_lib.lp_multiband_ws_bytes(*case) == _cabi.multiband_ws_bytes(*case), case
    assert _cabi.multiband_ws_bytes(1, 1, 1, 1, 5) == 16            # no level above the image: nothing to keep, never 0 bytes
    assert _cabi.multiband_ws_bytes(4, 300, 300, 3, 0) == 16
    assert _cabi.multiband_ws_bytes(1, 1, 2, 1, 1) == 16            # one pixel: 3 floats
    pix = 360 * 640 + 180 * 320 + 90 * 160 + 45 * 80 + 23 * 40
    assert _cabi.multiband_ws_bytes(81, 720, 1280, 3, 5) == 81 * pix * 7 * 4 == hip_lib.lp_multiband_ws_bytes(81, 720, 1280, 3, 5)
    assert 0.6e9 < 81 * pix * 7 * 4 < multiband.WS_CAP_BYTES == 1 << 30
    E, U = _cabi.LP_E_INVALID, _cabi.LP_E_UNSUPPORTED
    for bad in ((0, 8, 8, 3, 5), (-1, 8, 8, 3, 5), (1, 0, 8, 3, 5), (1, 8, 0, 3, 5), (1, 32769, 8, 3, 5), (1, 8, 32769, 3, 5),
                (1, 8, 8, 0, 5), (1, 8, 8, 65, 5), (1, 8, 8, 3, -1)):
        assert hip_lib.lp_multiband_ws_bytes(*bad) == E, bad
    assert hip_lib.lp_multiband_ws_bytes(65536, 8, 8, 3, 5) == U


def test_the_multiband_kernels_are_a_source_of_the_build():
    from lanpaint_amd import build
    assert "multiband_kernel.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "multiband_kernel.hip"))


# ---- the wrapper and the node ---------------------------------------------------------------------------------------------------------
def test_blend_multiband_refuses_cpu_tensors():
    img, mask = torch.zeros(2, 16, 16, 3), torch.zeros(2, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        multiband.blend_multiband(img, img.clone(), mask)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        multiband.blend_multiband(img, img.clone(), mask, levels=0)


def test_multiband_node_protocol_and_own_mappings():
    from lanpaint_amd import multiband_nodes
    node = multiband_nodes.LanPaint_MultibandBlend
    assert multiband_nodes.NODE_CLASS_MAPPINGS == {"LanPaint_MultibandBlend": node}
    assert multiband_nodes.NODE_DISPLAY_NAME_MAPPINGS == {"LanPaint_MultibandBlend": "LanPaint Multiband Blend"}
    types = node.INPUT_TYPES()
    req = types["required"]
    assert list(types) == ["required"] and list(req) == ["image1", "image2", "mask", "levels"]
    assert req["image1"][0] == "IMAGE" and req["image2"][0] == "IMAGE" and req["mask"][0] == "MASK"
    assert req["levels"][0] == "INT" and req["levels"][1] == {**req["levels"][1], "default": 5, "min": 0, "max": 12}
    assert node.RETURN_TYPES == ("IMAGE",) and node.FUNCTION == "blend" and node.CATEGORY == "image"
    assert callable(getattr(node, node.FUNCTION))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            node().blend(torch.zeros(2, 16, 16, 3), torch.zeros(2, 16, 16, 3), torch.zeros(2, 16, 16), 5)
