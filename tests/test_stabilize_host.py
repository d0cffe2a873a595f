"""The video mask stabilize, the parts that need no device: the restatement (tests/stabilize_ref.py) checked on its own -- its
distances against scipy, the properties the rule promises, as bits, and the flicker it exists to remove --, the two C entries'
argument checks (made before any HIP call), the node's protocol and the no-fallback errors.  Layouts, constants and names against
the header are tests/test_cabi_mirror.py's, for the whole C ABI."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, stabilize
from tests import stabilize_ref as ref
from tests.compare import _f32_bits as _bits

ONE = np.float32(1.0).view(np.uint32)


def _blobs(F, H, W, seed=0):
    """A disc that drifts and jitters, binary."""
    rng = np.random.default_rng([F, H, W, seed])
    yy, xx = np.mgrid[:H, :W]
    out = np.zeros((F, H, W), np.float32)
    for t in range(F):
        cy, cx = H / 2 + rng.normal(0, 1), W / 3 + 0.7 * t + rng.normal(0, 1)
        out[t] = (yy - cy) ** 2 + (xx - cx) ** 2 <= (min(H, W) / 3 + rng.normal(0, 1)) ** 2
    return out


# ---- the restatement on its own -------------------------------------------------------------------------------------------------------
def test_the_restatements_distances_are_scipys():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(5)
    for H, W, p in ((1, 1, 0.5), (1, 9, 0.3), (9, 1, 0.7), (17, 23, 0.05), (17, 23, 0.95), (40, 31, 0.5)):
        for _ in range(3):
            on = rng.random((H, W)) < p
            on.flat[rng.integers(on.size)] = False
            want = np.rint(ndimage.distance_transform_edt(on) ** 2).astype(np.int64)
            assert (ref.d2_exact(on) == want).all(), (H, W, p)
    mask = _blobs(3, 20, 30)
    q = ref.signed_d2(mask)
    for t in range(3):
        fg = mask[t] >= 0.5
        sd = ndimage.distance_transform_edt(fg) - ndimage.distance_transform_edt(~fg)
        assert (np.sign(q[t]) * np.sqrt(np.abs(q[t])) == sd).all()
        assert (q[t][fg] >= 1).all() and (q[t][~fg] <= -1).all()


def test_signed_d2_binarises_as_the_edt_does_and_marks_empty_and_full_frames():
    v = np.float32(0.5)
    frame = np.array([[0.0, np.nextafter(v, np.float32(0)), v, np.nextafter(v, np.float32(1)), np.nan, np.inf, -np.inf, 1.0]],
                     dtype=np.float32)
    assert (ref.signed_d2_frame(frame) > 0).tolist() == [[False, False, True, True, False, True, False, True]]
    assert ref.signed_d2_frame(frame).tolist() == [[-4, -1, 1, 1, -1, 1, -1, 1]]
    empty, full = np.zeros((3, 4), np.float32), np.ones((3, 4), np.float32)
    assert (ref.signed_d2_frame(empty) == -ref.Q_FAR).all() and (ref.signed_d2_frame(full) == ref.Q_FAR).all()
    assert ref.Q_FAR == _cabi.LP_STAB_Q_FAR == 1 << 30 > 2 * 16383 ** 2 and ref.SD_CAP == _cabi.LP_STAB_SD_CAP == 64.0
    planes = np.array([[[[0, 1, 4]], [[2, 0, 0]]], [[[-1, -1, -1]], [[0, 0, 0]]], [[[0, 0, 0]], [[-1, -1, -1]]]])
    assert ref.signed_from_planes(planes).tolist() == [[[2, -1, -4]], [[-ref.Q_FAR] * 3], [[ref.Q_FAR] * 3]]


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 1, 7), (3, 7, 1), (9, 5, 9), (24, 12, 17)], ids=lambda s: "x".join(map(str, s)))
def test_the_restatement_keeps_what_the_rule_promises(shape):
    F, H, W = shape
    rng = np.random.default_rng(list(shape))
    soft = rng.random(shape, dtype=np.float32)
    binar = (soft >= np.float32(0.5)).astype(np.float32)
    still = np.repeat(soft[:1], F, axis=0)
    for tm in range(4):
        for ts in (0, 1, 2, 5, 8):
            for feather in (0.0, 0.5, 3.0, 64.0):
                zero = ref.stabilize_ref(np.zeros(shape, np.float32), tm, ts, 0.0, feather)
                one = ref.stabilize_ref(np.ones(shape, np.float32), tm, ts, 0.0, feather)
                assert zero.dtype == np.float32 and zero.shape == shape
                assert (_bits(zero) == 0).all() and (_bits(one) == ONE).all(), (tm, ts, feather)
            # frames that are all equal: the binarised frame, whatever the radii
            assert (_bits(ref.stabilize_ref(still, tm, ts)) == _bits(np.repeat(binar[:1], F, axis=0))).all(), (tm, ts)
    assert (_bits(ref.stabilize_ref(soft, 0, 0)) == _bits(binar)).all()
    again = ref.stabilize_ref(soft, 2, 3, 0.5, 3.0)
    assert (again >= 0).all() and (again <= 1).all() and (_bits(again) == _bits(ref.stabilize_ref(soft, 2, 3, 0.5, 3.0))).all()


def test_the_median_is_the_middle_value_with_the_end_frames_replicated():
    q = np.array([5, -3, 9, -7, 1, 2, -8], dtype=np.int64).reshape(7, 1, 1)
    assert ref.temporal_median(q, 0).ravel().tolist() == [5, -3, 9, -7, 1, 2, -8]
    assert ref.temporal_median(q, 1).ravel().tolist() == [5, 5, -3, 1, 1, 1, -8]
    assert ref.temporal_median(q, 2).ravel().tolist() == [5, 5, 1, 1, 1, -7, -8]
    flat = q.ravel().tolist()
    for tm in range(4):                                              # and by the definition, one value at a time
        want = [sorted(flat[min(max(t + k, 0), 6)] for k in range(-tm, tm + 1))[tm] for t in range(7)]
        assert ref.temporal_median(q, tm).ravel().tolist() == want, tm
    s = np.array([1.0, 2.0, 4.0, 8.0]).reshape(4, 1, 1)
    assert ref.temporal_smooth(s, 1).ravel().tolist() == [1.25, 2.25, 4.5, 7.0]
    assert ref.temporal_smooth(s, 0).ravel().tolist() == [1.0, 2.0, 4.0, 8.0]
    assert ref.capped_distance(np.array([-ref.Q_FAR, -4097, -4096, -9, -2, 1, 4096, ref.Q_FAR])).tolist() == \
        [-64.0, -64.0, -64.0, -3.0, -np.sqrt(2.0), 1.0, 64.0, 64.0]
    u = np.array([-3.0, -1.5, 0.0, 1.5, 3.0, 4.0])
    assert ref.output(u, 0.0, 0.0).tolist() == [0, 0, 0, 1, 1, 1]
    assert ref.output(u, 1.5, 0.0).tolist() == [0, 0, 1, 1, 1, 1]
    assert ref.output(u, 0.0, 3.0).tolist() == [0.0, 0.25, 0.5, 0.75, 1.0, 1.0]


def test_a_short_dropout_or_blob_goes_with_the_median_and_stays_with_the_smoothing_alone():
    F, H, W = 9, 16, 20
    clean = np.zeros((F, H, W), np.float32)
    clean[:, 4:12, 5:15] = 1.0
    broken = clean.copy()
    broken[2] = 0.0                                                   # a dropped frame
    broken[5, 13:15, 0:3] = 1.0                                       # a stray blob
    broken[7:9] = 0.0                                                 # two frames long: beyond a median of radius 1
    out = ref.stabilize_ref(broken, 1, 0)
    assert (out[:7] == clean[:7]).all() and not out[7:].any()
    assert (ref.stabilize_ref(broken, 2, 0)[:7] == clean[:7]).all()
    assert not ref.stabilize_ref(broken, 0, 2)[2].all() and not (ref.stabilize_ref(broken, 0, 2)[2] == clean[2]).all()


@functools.lru_cache(maxsize=None)
def _jittered_disc():
    """The sequence the rule was tried on: 24 frames of 96 x 128, a disc of radius 22 moving (0.5, 2.0) pixels per frame, its
    centre jittering with sigma 1.5 and its radius with sigma 2, frames 7 and 15 empty, a stray 10 x 15 blob on frame 11."""
    F, H, W = 24, 96, 128
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[:H, :W]
    clean, noisy = np.zeros((F, H, W), np.float32), np.zeros((F, H, W), np.float32)
    for t in range(F):
        cy, cx = 40 + 0.5 * t, 36 + 2.0 * t
        clean[t] = (yy - cy) ** 2 + (xx - cx) ** 2 <= 22 ** 2
        jy, jx, jr = rng.normal(0, 1.5), rng.normal(0, 1.5), rng.normal(0, 2.0)
        noisy[t] = (yy - cy - jy) ** 2 + (xx - cx - jx) ** 2 <= (22 + jr) ** 2
    noisy[7] = noisy[15] = 0.0
    noisy[11, 5:15, 100:115] = 1.0
    return clean, noisy


def _iou(a, b):
    a, b = a > 0.5, b > 0.5
    return (a & b).sum(axis=(1, 2)) / np.maximum((a | b).sum(axis=(1, 2)), 1)


def _flicker(m, clean):
    changes = lambda v: float(((v[1:] > 0.5) != (v[:-1] > 0.5)).sum(axis=(1, 2)).mean())    # noqa: E731
    return changes(m) - changes(clean)


def test_the_rule_removes_the_flicker_of_a_jittered_disc():
    clean, noisy = _jittered_disc()
    out = ref.stabilize_ref(noisy, 1, 2)
    iou_in, iou_out = _iou(noisy, clean), _iou(out, clean)
    f_in, f_out = _flicker(noisy, clean), _flicker(out, clean)
    print("IoU in mean/min", iou_in.mean(), iou_in.min(), "out mean/min", iou_out.mean(), iou_out.min(), "flicker", f_in, f_out)
    assert iou_in.min() == 0.0 and iou_out.min() > 0.5               # both empty frames are filled, the blob is gone
    assert not out[11, 5:15, 100:115].any()
    assert f_in > 0 and f_out < f_in / 4
    alone = ref.stabilize_ref(noisy, 0, 2)                            # the smoothing alone does not repair a dropout
    assert _iou(alone, clean).min() < 0.5


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_stabilize_entries_reject_bad_arguments_without_a_device(hip_lib):
    C, E = ctypes, _cabi.LP_E_INVALID
    p, q = C.c_void_p(256), C.c_void_p(512)                          # never dereferenced: validation comes before any HIP call
    side = _cabi.LP_VMASK_MAX_SIDE
    for bad in ((None, 2, 8, 8, q), (p, 2, 8, 8, None), (p, 2, 8, 8, p), (p, 0, 8, 8, q), (p, -1, 8, 8, q), (p, 2, 0, 8, q),
                (p, 2, 8, 0, q), (p, 2, side + 1, 8, q), (p, 2, 8, side + 1, q), (p, 2, -5, 8, q)):
        assert hip_lib.lp_mask_signed_d2(*bad, None) == E, bad
    M = _cabi.LpStabilizeDesc
    assert hip_lib.lp_mask_stabilize(None, None) == E
    good = dict(frames=5, height=40, width=150, median_radius=1, smooth_radius=2, grow=0.0, feather=0.0, q=p, out=q)
    nan, inf = float("nan"), float("inf")
    for change in ({"frames": 0}, {"frames": -1}, {"height": 0}, {"height": side + 1}, {"width": 0}, {"width": side + 1},
                   {"median_radius": -1}, {"median_radius": 4}, {"smooth_radius": -1}, {"smooth_radius": 9}, {"grow": 256.5},
                   {"grow": -256.5}, {"grow": nan}, {"grow": inf}, {"grow": -inf}, {"feather": -0.25}, {"feather": 64.5},
                   {"feather": nan}, {"feather": inf}, {"q": None}, {"out": None}, {"out": p}):
        assert hip_lib.lp_mask_stabilize(C.byref(M(**{**good, **change})), None) == E, change
    assert hip_lib.lp_mask_stabilize(C.byref(M(**{**good, "frames": (1 << 30) + 1})), None) == _cabi.LP_E_UNSUPPORTED


def test_the_stabilize_kernels_are_a_source_of_the_build():
    from lanpaint_amd import build
    assert "stabilize_kernel.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "stabilize_kernel.hip"))


# ---- the wrapper and the node ---------------------------------------------------------------------------------------------------------
def test_stabilize_refuses_cpu_tensors_and_bad_arguments():
    mask = torch.zeros(4, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stabilize.stabilize_masks(mask)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stabilize.stabilize_q(torch.zeros(4, 16, 16, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stabilize.stabilize_masks(mask.numpy())
    # the numbers are checked before the tensor is looked at
    for bad in (dict(median=-1), dict(median=4), dict(median=1.0), dict(median=True), dict(smooth=-1), dict(smooth=9),
                dict(smooth=2.0), dict(grow=256.5), dict(grow=-257), dict(grow=float("nan")), dict(grow="1"),
                dict(feather=-0.5), dict(feather=64.25), dict(feather=float("nan")), dict(feather=None)):
        with pytest.raises(ValueError):
            stabilize.stabilize_masks(mask, **bad)
        with pytest.raises(ValueError):
            stabilize.stabilize_q(torch.zeros(4, 16, 16, dtype=torch.int32), **bad)
    for inside in (dict(median=0, smooth=0), dict(median=3, smooth=8, grow=-256, feather=64), dict(grow=256.0, feather=0)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            stabilize.stabilize_masks(mask, **inside)


def test_stabilize_node_protocol_and_own_mappings():
    from lanpaint_amd import stabilize_nodes
    node = stabilize_nodes.LanPaint_VideoMaskStabilize
    assert stabilize_nodes.NODE_CLASS_MAPPINGS == {"LanPaint_VideoMaskStabilize": node}
    assert stabilize_nodes.NODE_DISPLAY_NAME_MAPPINGS == {"LanPaint_VideoMaskStabilize": "LanPaint Video Mask Stabilize"}
    types = node.INPUT_TYPES()
    req = types["required"]
    assert list(types) == ["required"] and list(req) == ["mask", "median_radius", "smooth_radius", "grow", "feather"]
    assert req["mask"][0] == "MASK"
    assert req["median_radius"][0] == "INT" and req["median_radius"][1] == {**req["median_radius"][1], "default": 1, "min": 0, "max": 3}
    assert req["smooth_radius"][0] == "INT" and req["smooth_radius"][1] == {**req["smooth_radius"][1], "default": 2, "min": 0, "max": 8}
    assert req["grow"][0] == "FLOAT" and req["grow"][1] == {**req["grow"][1], "default": 0.0, "min": -256.0, "max": 256.0}
    assert req["feather"][0] == "FLOAT" and req["feather"][1] == {**req["feather"][1], "default": 0.0, "min": 0.0, "max": 64.0}
    for name in req:
        assert len(req[name][1]["tooltip"]) > 20, name
    assert "does not repair dropped frames" in req["smooth_radius"][1]["tooltip"]
    for word in ("segmenter", "video mask editor", "mask refine", "encode", "Detailer"):
        assert word in node.DESCRIPTION, word
    assert node.RETURN_TYPES == ("MASK",) and node.FUNCTION == "stabilize" and node.CATEGORY == "mask"
    assert callable(getattr(node, node.FUNCTION))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            node().stabilize(torch.zeros(4, 16, 16), 1, 2, 0.0, 0.0)
