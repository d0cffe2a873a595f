"""The video mask propagate, the parts that need no device: the restatement (tests/propagate_ref.py) checked on its own -- the
properties the rule promises, as bits, and the one quality condition it has to meet on moving-disc scenes --, the C entries'
argument checks (made before any HIP call), the node's protocol and the no-fallback errors.  Layouts, constants and names against
the header are tests/test_cabi_mirror.py's, for the whole C ABI."""
import ctypes
import os

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi
from tests import propagate_ref as ref
from tests.compare import _f32_bits as _bits, _iou
from tests.propagate_scenes import SCENES, disc_scene, texture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = np.float32(1.0).view(np.uint32)


# ---- the restatement on its own -------------------------------------------------------------------------------------------------------
def test_luma_codes_and_pyramids_follow_the_rule():
    v = np.array([-1.0, 0.0, 0.5 / 255, 1.5 / 255, 0.5, 1.0, 2.0, np.nan, np.inf, -np.inf], np.float32)
    assert ref.codes(v).tolist() == [0, 0, 1, 2, 128, 255, 255, 0, 255, 0]
    rgb = np.array([[[[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 1.0, 1.0]]]], np.float32)
    assert ref.luma(rgb).tolist() == [[[(77 * 255 + 128) >> 8, (150 * 255 + 128) >> 8, (29 * 255 + 128) >> 8, 255]]]
    assert ref.luma(rgb[..., :2]).tolist() == [[[255, 0, 0, 255]]] and ref.luma(rgb[..., :1]).tolist() == [[[255, 0, 0, 255]]]
    a = np.arange(15, dtype=np.uint8).reshape(3, 5) * 10
    assert ref.down_luma(a).tolist() == [[(0 + 10 + 50 + 60 + 2) >> 2, (20 + 30 + 70 + 80 + 2) >> 2, (40 + 40 + 90 + 90 + 2) >> 2],
                                         [(100 + 110) * 2 + 2 >> 2, (120 + 130) * 2 + 2 >> 2, 140]]
    m = np.zeros((5, 9), np.uint8)
    m[4, 8] = m[0, 3] = 1
    pyr = ref.pyramid(m, 4, ref.down_mask)
    assert [p.shape for p in pyr] == [(5, 9), (3, 5), (2, 3), (1, 2)]
    assert pyr[1].tolist() == [[0, 1, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 1]] and pyr[3].tolist() == [[1, 1]]
    for l, p in enumerate(pyr):
        assert p.shape == _cabi.prop_level_shape(5, 9, l)


def test_one_frame_empty_full_and_equal_frames():
    rng = np.random.default_rng(3)
    H, W = 23, 33
    soft = rng.random((H, W), dtype=np.float32)
    binar = (soft >= np.float32(0.5)).astype(np.float32)
    one = ref.propagate_ref(rng.random((1, H, W, 3), dtype=np.float32), soft, 0, 3, 2, 8)
    assert one.dtype == np.float32 and (_bits(one[0]) == _bits(binar)).all()
    video = rng.random((4, H, W, 3), dtype=np.float32)
    for key in (0, 2, 3):
        assert (_bits(ref.propagate_ref(video, np.zeros((H, W), np.float32), key, 3, 2, 8)) == 0).all()
        assert (_bits(ref.propagate_ref(video, np.ones((H, W), np.float32), key, 3, 2, 8)) == ONE).all()
    still = np.repeat(video[:1], 4, axis=0)
    for levels, search, smooth in ((1, 1, 0), (3, 2, 8), (6, 7, 64)):
        got = ref.propagate_ref(still, soft, 1, levels, search, smooth)
        assert (_bits(got) == _bits(np.repeat(binar[None], 4, axis=0))).all(), (levels, search, smooth)
    const = np.full((3, H, W, 1), 0.25, np.float32)                    # every cost ties: the zero vector wins
    assert (_bits(ref.propagate_ref(const, soft, 0, 3, 2, 0)) == _bits(np.repeat(binar[None], 3, axis=0))).all()


@pytest.mark.parametrize("shift", [(2, -1), (-3, 5)], ids=str)
def test_a_whole_pixel_shift_is_tracked_exactly(shift):
    """A u8 random texture (1 / f^1.2, so that the coarse levels have something to hold on to: white noise averages away there)
    shifted by whole pixels per frame; the mask's travel plus the search reach stays inside the image."""
    F, H, W = 5, 96, 112
    big = (np.round(texture((7, 9)) * 255) / 255).astype(np.float32)
    images = np.stack([big[40 - shift[0] * t: 40 - shift[0] * t + H, 40 - shift[1] * t: 40 - shift[1] * t + W] for t in range(F)])
    mask = np.zeros((H, W), np.float32)
    mask[36:60, 40:70] = 1
    out = ref.propagate_ref(images[..., None], mask, 0, 3, 2, 8)
    for t in range(F):
        assert (_bits(out[t]) == _bits(np.roll(mask, (shift[0] * t, shift[1] * t), (0, 1)))).all(), t


def test_the_chains_before_and_after_a_middle_key_frame_are_independent():
    images, discs = disc_scene(7, (1.3, -0.7), (0.3, -0.4), 14, (48, 64), seed=5)
    mask = discs[3].astype(np.float32)
    whole = ref.propagate_ref(images, mask, 3, 3, 2, 8)
    assert (_bits(whole[3:]) == _bits(ref.propagate_ref(images[3:], mask, 0, 3, 2, 8))).all()
    assert (_bits(whole[:4]) == _bits(ref.propagate_ref(images[:4], mask, 3, 3, 2, 8))).all()
    other = images.copy()
    other[:3] = other[:3][:, ::-1]                                    # other frames in front of the key: the frames behind it stay
    assert (_bits(ref.propagate_ref(other, mask, 3, 3, 2, 8)[3:]) == _bits(whole[3:])).all()
    per_frame = np.zeros((7, 96, 128), np.float32)
    per_frame[3] = mask                                               # [F, H, W]: the key frame's mask is the one that is read
    assert (_bits(ref.propagate_ref(images, per_frame, 3, 3, 2, 8)) == _bits(whole)).all()


@pytest.mark.parametrize("name", list(SCENES))
def test_the_mask_follows_a_moving_disc(name):
    """The quality condition: at the last frame the propagated mask is more than half way from the unmoved key mask to the truth."""
    images, discs = disc_scene(*SCENES[name])
    out = ref.propagate_ref(images, discs[0].astype(np.float32), 0, 3, 2, 8)
    static, got = _iou(discs[0], discs[-1]), _iou(out[-1] >= 0.5, discs[-1])
    print(name, "IoU", got, "static", static, "floor", static + (1 - static) / 2)
    assert got > static + (1 - static) / 2


def test_the_pieces_of_the_rule_one_at_a_time():
    # fill: the floor of the mean, Jacobi, three rings at most; what stays invalid keeps its own value
    vec = np.zeros((1, 6, 2), np.int64)
    valid = np.zeros((1, 6), bool)
    vec[0, 0], valid[0, 0] = (-5, 7), True
    vec[0, 5] = (32, -32)
    assert ref.fill(vec, valid)[0].tolist() == [[-5, 7]] * 4 + [[0, 0], [32, -32]]
    vec2, valid2 = np.zeros((2, 2, 2), np.int64), np.array([[True, True], [True, False]])
    vec2[0, 0], vec2[0, 1], vec2[1, 0] = (-1, 1), (-2, 2), (0, 2)
    assert ref.fill(vec2, valid2)[1, 1].tolist() == [-1, 2]           # floor((2 * -3 + 3) / 6) = -1, floor((10 + 3) / 6) = 2
    v = np.arange(18).reshape(3, 3, 2)
    assert ref.median3(v)[1, 1].tolist() == [8, 9] and ref.median3(v)[0, 0].tolist() == [2, 3]
    # the per-pixel vector: block centres at 8 b + 3.5
    field = np.zeros((2, 2, 2), np.int64)
    field[:, 1] = (16, -32)
    V = ref.pixel_vectors(field, 16, 16)
    assert V[0, 0].tolist() == [0, 0] and V[0, 15].tolist() == [16, -32] and V[5, 3, 0] == 0 and V[5, 12, 0] == 16
    assert V[5, 7].tolist() == [(9 * 0 + 7 * 16 * 16 + 128) >> 8, (16 * 7 * -32 + 128) >> 8]
    # bil and the advance of a zero field
    P = ref.key_positions(5, 7)
    assert (ref.bil(P, P[..., 0], P[..., 1]) == 256 * P).all()
    bits = np.zeros((5, 7), np.uint8)
    bits[2, 3] = 1
    assert int(ref.bil(bits, np.array(2 * 16 + 8), np.array(3 * 16 + 4))) == 8 * 12
    P_t, c = ref.advance(P, np.zeros((1, 1, 2), np.int64), bits)
    assert (P_t == P).all() and (c == 256 * bits.astype(np.int64)).all()
    # the match: a shifted ramp under a full mask, the tie-break and the sub-pixel step
    yy, xx = np.mgrid[:16, :24]
    Ys = ((yy * 7 + xx * 5) % 256).astype(np.uint8)
    full = np.ones((16, 24), np.uint8)
    vec, ok = ref.match_level(Ys, Ys, full, None, 2, 8, True)
    assert ok.all() and not vec.any()
    vec, ok = ref.match_level(np.full((16, 24), 9, np.uint8), np.full((16, 24), 200, np.uint8), full, None, 2, 0, True)
    assert ok.all() and not vec.any()                                  # every cost ties: the least |o|, then the least idx
    few = np.zeros((16, 24), np.uint8)
    few[0:4, 4:8] = 1                                                  # 16 pixels inside the windows of blocks (0, 0) and (0, 1)
    few[3, 7] = 0
    assert not ref.match_level(Ys, Ys, few, None, 2, 8, True)[1].any()
    few[3, 7] = 1
    assert ref.match_level(Ys, Ys, few, None, 2, 8, True)[1].tolist() == [[True, True, False], [False, False, False]]


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_propagate_entries_reject_bad_arguments_without_a_device(hip_lib):
    C, E, U = ctypes, _cabi.LP_E_INVALID, _cabi.LP_E_UNSUPPORTED
    p, q, r = C.c_void_p(256), C.c_void_p(512), C.c_void_p(1024)      # never dereferenced: validation comes before any HIP call
    side = _cabi.LP_VMASK_MAX_SIDE
    for bad in ((0, 8, 8, 3), (-1, 8, 8, 3), (1, 0, 8, 3), (1, 8, 0, 3), (1, side + 1, 8, 3), (1, 8, side + 1, 3), (1, 8, 8, 0),
                (1, 8, 8, 7)):
        assert hip_lib.lp_prop_pyramid_ws_bytes(*bad) == E, bad
    for (F, H, W, L) in ((1, 1, 1, 1), (3, 5, 9, 4), (2, 70, 130, 6), (1, side, side, 6)):
        assert hip_lib.lp_prop_pyramid_ws_bytes(F, H, W, L) == _cabi.prop_pyramid_ws_bytes(F, H, W, L)
    assert _cabi.prop_pyramid_ws_bytes(1, 5, 9, 4) == 48 + 16 + 16 + 16 and _cabi.prop_level_offset(70, 130, 1) == 9104

    assert hip_lib.lp_prop_luma(None, None) == E
    good = dict(frames=3, height=40, width=70, channels=3, levels=4, image=p, pyramid=q)
    for change in ({"frames": 0}, {"frames": -2}, {"height": 0}, {"height": side + 1}, {"width": 0}, {"width": side + 1},
                   {"channels": 0}, {"channels": _cabi.LP_DETAIL_MAX_CHANNELS + 1}, {"levels": 0}, {"levels": 7}, {"image": None},
                   {"pyramid": None}):
        assert hip_lib.lp_prop_luma(C.byref(_cabi.LpPropLumaDesc(**{**good, **change})), None) == E, change
    assert hip_lib.lp_prop_luma(C.byref(_cabi.LpPropLumaDesc(**{**good, "frames": 65536})), None) == U

    for bad in ((None, 8, 8, 3, q, r), (p, 8, 8, 3, None, r), (p, 0, 8, 3, q, r), (p, 8, side + 1, 3, q, r), (p, 8, 8, 0, q, r),
                (p, 8, 8, 7, q, r), (p, 8, 8, 3, q, p)):
        assert hip_lib.lp_prop_key_mask(*bad, None) == E, bad

    assert hip_lib.lp_prop_match(None, None) == E
    good = dict(height=40, width=70, levels=3, level=1, search=2, smooth=8, src=p, tgt=q, mask=r, parent=C.c_void_p(2048),
                vec=C.c_void_p(4096), valid=C.c_void_p(8192))
    for change in ({"height": 0}, {"width": side + 1}, {"levels": 0}, {"levels": 7}, {"level": -1}, {"level": 3}, {"search": 0},
                   {"search": 8}, {"smooth": -1}, {"smooth": 65}, {"src": None}, {"tgt": None}, {"mask": None}, {"vec": None},
                   {"valid": None}, {"parent": None}, {"level": 2}, {"parent": C.c_void_p(4096)}):
        assert hip_lib.lp_prop_match(C.byref(_cabi.LpPropMatchDesc(**{**good, **change})), None) == E, change

    v, ok, out = C.c_void_p(256), C.c_void_p(512), C.c_void_p(1024)
    grid = _cabi.LP_PROP_MAX_GRID
    for bad in ((None, ok, 4, 4, out), (v, None, 4, 4, out), (v, ok, 4, 4, None), (v, ok, 4, 4, v), (v, ok, 0, 4, out),
                (v, ok, 4, 0, out), (v, ok, grid + 1, 4, out), (v, ok, 4, grid + 1, out)):
        assert hip_lib.lp_prop_fill(*bad, None) == E, bad

    assert hip_lib.lp_prop_advance(None, None) == E
    good = dict(height=40, width=70, levels=3, vec=p, pos_src=q, key=r, pos_dst=C.c_void_p(2048), out=C.c_void_p(4096),
                mask_pyramid=C.c_void_p(8192))
    for change in ({"height": 0}, {"height": side + 1}, {"width": 0}, {"levels": 0}, {"levels": 7}, {"vec": None}, {"key": None},
                   {"pos_dst": None}, {"out": None}, {"mask_pyramid": None}, {"pos_dst": q}, {"mask_pyramid": r}):
        assert hip_lib.lp_prop_advance(C.byref(_cabi.LpPropAdvanceDesc(**{**good, **change})), None) == E, change


def test_the_propagate_kernels_are_built_and_the_header_says_the_words():
    header = open(os.path.join(ROOT, "include", "lanpaint_hip.h")).read()
    from lanpaint_amd import build
    assert "propagate_kernel.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "propagate_kernel.hip"))
    for word in ("LP_PROP_MIN_PIXELS", "cost << 12", "inside an int32", "inside 32 bits"):
        assert word in header, word


# ---- the wrapper and the node ---------------------------------------------------------------------------------------------------------
def test_propagate_refuses_cpu_tensors_and_bad_arguments():
    from lanpaint_amd import propagate
    images, mask = torch.zeros(4, 16, 16, 3), torch.zeros(16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        propagate.propagate_masks(images, mask)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        propagate.propagate_masks(images.numpy(), mask)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        propagate.luma_pyramids(images, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        propagate.key_mask(mask, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        propagate.fill_median(torch.zeros(2, 2, 2, dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        propagate.advance(torch.zeros(2, 2, 2, dtype=torch.int32), None, torch.zeros(16, 16, dtype=torch.uint8), 3)
    row = torch.zeros(_cabi.prop_pyramid_ws_bytes(1, 16, 16, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        propagate.match_level(row, row, row, 16, 16, 3, 2)
    # the numbers are checked before the tensors are looked at
    for bad in (dict(levels=0), dict(levels=7), dict(levels=2.0), dict(levels=True), dict(search=0), dict(search=8), dict(search="2"),
                dict(smooth=-1), dict(smooth=65), dict(smooth=8.0), dict(smooth=None)):
        with pytest.raises(ValueError):
            propagate.propagate_masks(images, mask, **bad)
    for inside in (dict(levels=1, search=1, smooth=0), dict(levels=6, search=7, smooth=64)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            propagate.propagate_masks(images, mask, **inside)
    assert propagate.WS_CAP_BYTES == 1 << 30
    assert (propagate.MAX_LEVELS, propagate.MAX_SEARCH, propagate.MAX_SMOOTH, propagate.MAX_SIDE) == (6, 7, 64, _cabi.LP_VMASK_MAX_SIDE)
    assert sum(1 for _ in open(propagate.__file__)) <= 900


def test_propagate_node_protocol_and_own_mappings():
    from lanpaint_amd import propagate_nodes
    node = propagate_nodes.LanPaint_VideoMaskPropagate
    assert propagate_nodes.NODE_CLASS_MAPPINGS == {"LanPaint_VideoMaskPropagate": node}
    assert propagate_nodes.NODE_DISPLAY_NAME_MAPPINGS == {"LanPaint_VideoMaskPropagate": "LanPaint Video Mask Propagate"}
    types = node.INPUT_TYPES()
    req = types["required"]
    assert list(types) == ["required"] and list(req) == ["image", "mask", "key_frame", "levels", "search", "smooth"]
    assert req["image"][0] == "IMAGE" and req["mask"][0] == "MASK"
    assert req["key_frame"][0] == "INT" and req["key_frame"][1] == {**req["key_frame"][1], "default": 0, "min": 0}
    assert req["levels"][0] == "INT" and req["levels"][1] == {**req["levels"][1], "default": 4, "min": 1, "max": 6}
    assert req["search"][0] == "INT" and req["search"][1] == {**req["search"][1], "default": 2, "min": 1, "max": 7}
    assert req["smooth"][0] == "INT" and req["smooth"][1] == {**req["smooth"][1], "default": 8, "min": 0, "max": 64}
    for name in req:
        assert len(req[name][1]["tooltip"]) > 20, name
    for word in ("one frame", "motion", "stabilize", "mask refine", "encode", "Detailer", "One keyframe", "occlusion", "drift"):
        assert word in node.DESCRIPTION, word
    assert node.RETURN_TYPES == ("MASK",) and node.FUNCTION == "propagate" and node.CATEGORY == "mask"
    assert callable(getattr(node, node.FUNCTION))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            node().propagate(torch.zeros(4, 16, 16, 3), torch.zeros(16, 16), 0, 4, 2, 8)
