"""The Detailer colour match, the parts that need no device: the three C entries' argument checks (made before any HIP call), the
node's protocol, the no-fallback errors, and the plain restatement (tests/color_ref.py) checked on its own.  Layouts, constants
and names against the header are tests/test_cabi_mirror.py's, for the whole C ABI."""
import ctypes
import os

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, detail_color
from tests import color_ref


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_color_stats_rejects_bad_arguments_without_a_device(hip_lib):
    C, E, U, A = ctypes, _cabi.LP_E_INVALID, _cabi.LP_E_UNSUPPORTED, _cabi.LP_E_ALIGN
    p = C.c_void_p(256)                                    # never dereferenced: validation comes before any HIP call
    S = _cabi.LpColorStatsDesc
    assert hip_lib.lp_color_stats(None, None) == E
    ws = _cabi.lp_color_ws_bytes(2, 40, 150, 3)
    good = dict(batch=2, height=40, width=150, channels=3, mask_batch=1, margin=8, detail=p, reference=p, mask=p, stats=p,
                workspace=p, workspace_bytes=ws)
    for change in ({"batch": 0}, {"batch": -1}, {"height": 0}, {"height": _cabi.LP_DETAIL_MAX_SIDE + 1}, {"width": 0},
                   {"width": _cabi.LP_DETAIL_MAX_SIDE + 1}, {"channels": 0}, {"channels": _cabi.LP_DETAIL_MAX_CHANNELS + 1},
                   {"margin": -1}, {"margin": 26}, {"mask_batch": 0}, {"mask_batch": 3}, {"detail": None}, {"reference": None},
                   {"stats": None}, {"workspace": None}, {"workspace_bytes": ws - 1}, {"workspace_bytes": 0}):
        assert hip_lib.lp_color_stats(C.byref(S(**{**good, **change})), None) == E, change
    for unaligned in (260, 264, 257):
        assert hip_lib.lp_color_stats(C.byref(S(**{**good, "workspace": unaligned})), None) == A, unaligned
    big = {**good, "batch": 65536, "workspace_bytes": _cabi.lp_color_ws_bytes(65536, 40, 150, 3)}
    assert hip_lib.lp_color_stats(C.byref(S(**big)), None) == U
    assert hip_lib.lp_color_stats(C.byref(S(**{**big, "mask_batch": 65536})), None) == U
    # the limits themselves are inside: margin 25, 64 channels, the largest side (the next refusal is the short workspace)
    edge = {**good, "margin": 25, "channels": 64, "height": _cabi.LP_DETAIL_MAX_SIDE, "workspace_bytes": 1}
    assert hip_lib.lp_color_stats(C.byref(S(**edge)), None) == E
    assert hip_lib.lp_color_stats(C.byref(S(**{**edge, "workspace": 264})), None) == A     # alignment is looked at before the length


def test_color_fit_rejects_bad_arguments_without_a_device(hip_lib):
    C, E, U = ctypes, _cabi.LP_E_INVALID, _cabi.LP_E_UNSUPPORTED
    p = C.c_void_p(256)
    F = _cabi.LpColorFitDesc
    assert hip_lib.lp_color_fit(None, None) == E
    good = dict(batch=12, channels=3, clip_frames=4, smooth=3, method=_cabi.LP_COLOR_METHOD_MEAN_STD, reserved0=0, strength=0.5,
                stats=p, coef=p)
    for change in ({"batch": 0}, {"channels": 0}, {"channels": 65}, {"clip_frames": -1}, {"clip_frames": 5}, {"clip_frames": 24},
                   {"smooth": -1}, {"smooth": 2}, {"smooth": 128}, {"smooth": 130}, {"smooth": 131}, {"method": 2}, {"method": -1},
                   {"strength": -0.01}, {"strength": 1.01}, {"strength": float("nan")}, {"stats": None}, {"coef": None}):
        assert hip_lib.lp_color_fit(C.byref(F(**{**good, **change})), None) == E, change
    assert hip_lib.lp_color_fit(C.byref(F(**{**good, "batch": 65536})), None) == U


def test_color_apply_rejects_bad_arguments_without_a_device(hip_lib):
    C, E, U = ctypes, _cabi.LP_E_INVALID, _cabi.LP_E_UNSUPPORTED
    p = C.c_void_p(256)
    A = _cabi.LpColorApplyDesc
    assert hip_lib.lp_color_apply(None, None) == E
    good = dict(batch=2, height=40, width=150, channels=3, detail=p, coef=p, out=p)
    for change in ({"batch": 0}, {"height": 0}, {"height": _cabi.LP_DETAIL_MAX_SIDE + 1}, {"width": -3},
                   {"width": _cabi.LP_DETAIL_MAX_SIDE + 1}, {"channels": 0}, {"channels": 65}, {"detail": None}, {"coef": None},
                   {"out": None}):
        assert hip_lib.lp_color_apply(C.byref(A(**{**good, **change})), None) == E, change
    assert hip_lib.lp_color_apply(C.byref(A(**{**good, "batch": 65536})), None) == U


def test_the_color_kernels_are_a_source_of_the_build():
    from lanpaint_amd import build
    assert "color_kernel.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "color_kernel.hip"))


# ---- the wrappers and the node --------------------------------------------------------------------------------------------------------
def test_color_functions_refuse_cpu_tensors():
    img, mask = torch.zeros(2, 16, 16, 3), torch.zeros(2, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        detail_color.match(img, img, mask)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        detail_color.color_stats(img, img, mask, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        detail_color.color_fit(torch.zeros(2, 13, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        detail_color.color_apply(img, torch.zeros(2, 3, 2))


def test_color_parameter_checks_raise_value_error():
    for kw in ({"method": "histogram"}, {"strength": -0.1}, {"strength": 1.5}, {"strength": "1"}, {"smooth": 2}, {"smooth": 131},
               {"smooth": -1}, {"smooth": 1.0}, {"clip_frames": 5}, {"clip_frames": -2}, {"clip_frames": 2.0}):
        args = {"batch": 12, "method": "mean_std", "strength": 1.0, "smooth": 1, "clip_frames": 0, **kw}
        with pytest.raises(ValueError):
            detail_color._check_fit(**args)
    detail_color._check_fit(12, "mean", 0, 0, 4)
    detail_color._check_fit(12, "mean_std", 1, 129, 12)
    for margin in (-1, 26, 2.0, None):
        with pytest.raises(ValueError):
            detail_color._check_margin(margin)
    detail_color._check_margin(0), detail_color._check_margin(25)


def test_color_node_protocol_and_own_mappings():
    from lanpaint_amd import detail_color_nodes
    node = detail_color_nodes.LanPaint_DetailerColorMatch
    assert detail_color_nodes.NODE_CLASS_MAPPINGS == {"LanPaint_DetailerColorMatch": node}
    assert set(detail_color_nodes.NODE_DISPLAY_NAME_MAPPINGS) == set(detail_color_nodes.NODE_CLASS_MAPPINGS)
    req = node.INPUT_TYPES()["required"]
    assert list(req) == ["image", "reference", "mask", "method", "strength", "margin", "smooth", "clip_frames"]
    assert req["image"][0] == "IMAGE" and req["reference"][0] == "IMAGE" and req["mask"][0] == "MASK"
    assert req["method"][0] == ["mean_std", "mean"]
    assert req["strength"][0] == "FLOAT" and req["strength"][1] == {**req["strength"][1], "default": 1.0, "min": 0.0, "max": 1.0,
                                                                    "step": 0.05}
    assert req["margin"][0] == "INT" and req["margin"][1] == {**req["margin"][1], "default": 8, "min": 0, "max": 25}
    assert req["smooth"][0] == "INT" and req["smooth"][1] == {**req["smooth"][1], "default": 1, "min": 0, "max": 129}
    assert req["clip_frames"][0] == "INT" and req["clip_frames"][1] == {**req["clip_frames"][1], "default": 0, "min": 0}
    assert "per region" in req["clip_frames"][1]["tooltip"]
    assert node.RETURN_TYPES == ("IMAGE",) and node.FUNCTION == "match" and node.CATEGORY == "image"
    assert callable(getattr(node, node.FUNCTION))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            node().match(torch.zeros(2, 16, 16, 3), torch.zeros(2, 16, 16, 3), torch.zeros(2, 16, 16))


# ---- the restatement on its own -------------------------------------------------------------------------------------------------------
def _block_mask(H, W):
    m = np.zeros((1, H, W), dtype=np.float32)
    m[0, H // 2 - max(1, H // 8): H // 2 + max(1, H // 8), W // 2 - max(1, W // 8): W // 2 + max(1, W // 8)] = 1.0
    return m


@pytest.mark.parametrize("shape", [(70, 150, 3), (17, 33, 4), (257, 300, 3)])
def test_the_restatement_recovers_an_affine_drift(shape):
    """d = fl(fl(0.8 r) + 0.1) and a centred block mask: the fitted output is r again.  The issue's bound is 8 x 2^-24; the
    restatement alone stays within 2 x 2^-24 (the drift's two roundings, about 2^-25 each at r < 1, come back magnified by
    1 / 0.8, and the map's own two roundings add 2^-25 each)."""
    H, W, C = shape
    rng = np.random.default_rng(H * 1000 + W)
    r = rng.random((2, H, W, C), dtype=np.float32)
    d = (r * np.float32(0.8)).astype(np.float32) + np.float32(0.1)
    mask = _block_mask(H, W)
    out = color_ref.match_ref(d, r, mask, "mean_std", 1.0, 2, 1, 0)
    err = float(np.abs(out.astype(np.float64) - r.astype(np.float64)).max())
    print(f"{shape}: max |out - r| = {err / 2.0 ** -24:.3f} x 2^-24")
    assert out.dtype == np.float32 and err <= 8 * 2.0 ** -24
    assert err <= 2 * 2.0 ** -24


def test_the_restatement_keep_rule_pooling_and_guards():
    # keep: a single element just above 0.5 drops its (2 margin + 1)^2 block, cut at the border; exactly 0.5 keeps
    m = np.zeros((1, 9, 11), dtype=np.float32)
    m[0, 0, 0], m[0, 5, 6] = np.nextafter(np.float32(0.5), np.float32(1.0)), 0.5
    keep = color_ref.keep_mask(m, 2, 3, 9, 11)
    assert keep.shape == (3, 9, 11) and not keep[:, :3, :3].any() and int((~keep[0]).sum()) == 9
    plain = np.array([[not (y <= 2 and x <= 2) for x in range(11)] for y in range(9)])
    assert (keep[1] == plain).all()
    assert color_ref.keep_mask(None, 8, 2, 4, 5).all()
    # pool: frames 0..3 of two clips; smooth 3 cuts the window at the clip's ends and never crosses into the other clip
    stats = np.zeros((8, 5))
    stats[:, 0] = 100
    stats[:, 1] = 100 * np.arange(8)                                # sum d: mean d = frame index
    stats[:, 2] = 0.0                                               # mean r = 0  ->  bias = -pooled mean d
    coef = color_ref.fit_ref(stats, "mean", 1.0, 3, 4)
    assert coef[:, 0, 0].tolist() == [1.0] * 8
    assert coef[:, 0, 1].tolist() == [-0.5, -1.0, -2.0, -2.5, -4.5, -5.0, -6.0, -6.5]
    assert color_ref.fit_ref(stats, "mean", 1.0, 0, 4)[:, 0, 1].tolist() == [-1.5] * 4 + [-5.5] * 4
    assert color_ref.fit_ref(stats, "mean", 1.0, 0, 0)[:, 0, 1].tolist() == [-3.5] * 8
    assert color_ref.fit_ref(stats, "mean", 0.0, 3, 4)[:, 0].tolist() == [[1.0, 0.0]] * 8
    # guards: n = 63 fits nothing, n = 64 does; a flat detail channel keeps gain 1; the gain is limited to [0.25, 4]
    def row(n, md, vd, mr, vr):
        return [n, n * md, n * mr, n * (vd + md * md), n * (vr + mr * mr)]
    few = color_ref.fit_ref(np.array([row(63, 0.5, 0.01, 0.25, 0.04), row(64, 0.5, 0.01, 0.25, 0.04)]), "mean_std", 1.0, 1, 0)
    assert few[0, 0].tolist() == [1.0, 0.0] and few[1, 0].tolist() == [2.0, -0.75]
    lim = color_ref.fit_ref(np.array([row(100, 0.5, 0.0, 0.25, 0.04), row(100, 0.5, 0.0001, 0.25, 1.0),
                                      row(100, 0.5, 1.0, 0.25, 0.0001)]), "mean_std", 1.0, 1, 0)
    assert lim[:, 0].tolist() == [[1.0, -0.25], [4.0, -1.75], [0.25, 0.125]]
