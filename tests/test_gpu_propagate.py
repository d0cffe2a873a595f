"""The video mask propagate on the MI355X (lanpaint_amd.propagate, csrc/propagate_kernel.hip) against the numpy restatement
tests/propagate_ref.py.  The rule is integer arithmetic throughout, so the device must give the restatement's values whatever tile,
block or chunk a launch uses: every comparison covers every element and has no tolerance.  Each stage is compared on its own (fed
with the restatement's inputs for that stage) and the whole chain as well."""

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, propagate, propagate_nodes
from tests import propagate_ref as ref
from tests.compare import _f32_bits as _bits, _same_bits, _same_ints as _same
from tests.device import _dev, _levels_of
from tests.inputs import BIG, MASKS, PLANES, VIDEOS, _advance_case, _disc, _rng, _soft, _video
from tests.motion_checks import _check_match

pytestmark = pytest.mark.gpu
ONE = np.float32(1.0).view(np.uint32)


# ---- stage 1 and 2: luma and pyramids ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2, 3, 4])
def test_luma_and_pyramids_equal_the_restatement(channels):
    for H, W in PLANES + [BIG]:
        for name, make in VIDEOS.items():
            images = make(3, H, W, channels)
            want = ref.luma(images)
            for levels in (1, 6):
                pyr = propagate.luma_pyramids(_dev(images), levels)
                assert pyr.dtype == torch.uint8 and tuple(pyr.shape) == (3, _cabi.prop_pyramid_ws_bytes(1, H, W, levels))
                got = _levels_of(pyr, H, W, levels)
                for f in range(3):
                    for lv, plane in enumerate(ref.pyramid(want[f], levels, ref.down_luma)):
                        _same(got[lv][f], plane, ("luma", (H, W), name, levels, f, lv))
                assert got[-1].shape[1:] == _cabi.prop_level_shape(H, W, levels - 1)
    assert _cabi.prop_level_shape(*BIG, 5) == (3, 5) and _cabi.prop_level_shape(23, 33, 5) == (1, 2)


@pytest.mark.parametrize("form", list(MASKS))
def test_key_mask_and_its_pyramid_equal_the_restatement(form):
    for H, W in PLANES + [BIG]:
        mask = MASKS[form](H, W)
        bits = ref.binarise(mask)
        for levels in (1, 3, 6):
            mpyr, out = propagate.key_mask(_dev(mask), levels)
            _same_bits(out.cpu().numpy(), bits.astype(np.float32), ("key mask", form, (H, W)))
            for lv, (g, w) in enumerate(zip(_levels_of(mpyr, H, W, levels), ref.pyramid(bits, levels, ref.down_mask))):
                _same(g[0], w, ("mask pyramid", form, (H, W), levels, lv))


# ---- stage 3: the match, the fill and median, the advance, each fed with the restatement's inputs -------------------------------------------
@pytest.mark.parametrize("search,smooth", [(1, 0), (2, 8), (7, 64)])
def test_match_equals_the_restatement_on_every_plane(search, smooth):
    for H, W in PLANES:
        for levels in (1, 3, 6):
            _check_match(H, W, levels, search, smooth, "random", "full" if (H + levels) % 2 else "disc", ((H, W), levels, search, smooth))


@pytest.mark.parametrize("mask", list(MASKS))
def test_match_equals_the_restatement_for_every_mask_and_image(mask):
    H, W = 23, 33
    for video in VIDEOS:
        trace = _check_match(H, W, 3, 2, 8, video, mask, (mask, video))
        if mask in ("empty", "one pixel", "15 pixels"):
            assert not trace[0][1].any() and not trace[0][2].any()    # no valid block at level 0: the zero field
        if mask == "16 pixels":
            assert trace[0][1][0, 0] and trace[0][1].sum() == 1
        if video == "constant" and mask == "full":
            assert trace[0][1].all() and not trace[0][0].any()        # every cost ties: the zero vector wins


def test_match_with_several_workgroups():
    _check_match(*BIG, 3, 2, 8, "random", "disc", BIG)
    _check_match(*BIG, 6, 7, 0, "random", "soft", BIG)


@pytest.mark.parametrize("grid", [(1, 1), (1, 7), (3, 5), (16, 16), (17, 33), (40, 50)], ids=lambda g: "x".join(map(str, g)))
def test_fill_and_median_equal_the_restatement(grid):
    gh, gw = grid
    for density in (0.0, 0.03, 0.3, 1.0):                              # 0.03: holes wider than the three passes reach
        rng = _rng(gh, gw, int(density * 100))
        vec = rng.integers(-7100, 7100, (gh, gw, 2)).astype(np.int32)
        valid = rng.random((gh, gw)) < density
        got = propagate.fill_median(_dev(vec), _dev(valid.astype(np.int32))).cpu().numpy()
        _same(got, ref.fill_median(vec, valid), (grid, density))


@pytest.mark.parametrize("scale", [0, 40, 7100])
def test_advance_equals_the_restatement(scale):
    for H, W in PLANES + [BIG]:
        vec, vec2, bits, P1, c1, P2, c2 = _advance_case(H, W, scale)
        for levels in (1, 6):
            pos1, out1, mp1 = propagate.advance(_dev(vec), None, _dev(bits), levels)
            pos2, out2, mp2 = propagate.advance(_dev(vec2), pos1, _dev(bits), levels)
            for pos, out, mp, P, c in ((pos1, out1, mp1, P1, c1), (pos2, out2, mp2, P2, c2)):
                _same(pos.cpu().numpy(), P, ("positions", (H, W), scale))
                _same_bits(out.cpu().numpy(), c.astype(np.float32) / np.float32(256), ("mask", (H, W), scale))
                want = ref.pyramid((c >= 128).astype(np.uint8), levels, ref.down_mask)
                for lv, g in enumerate(_levels_of(mp, H, W, levels)):
                    _same(g[0], want[lv], ("next bits", (H, W), scale, lv))


# ---- the whole chain ------------------------------------------------------------------------------------------------------------------
def _chain(images, mask, key, levels, search, smooth, what):
    want = ref.propagate_ref(images, mask, key, levels, search, smooth)
    got = propagate.propagate_masks(_dev(images), _dev(mask), key, levels, search, smooth)
    assert got.is_cuda and got.dtype == torch.float32
    _same_bits(got.cpu().numpy(), want, what)
    return want


@pytest.mark.parametrize("plane", PLANES + [BIG], ids=lambda s: "x".join(map(str, s)))
def test_the_chain_equals_the_restatement_bit_for_bit(plane):
    H, W = plane
    cases = [(3, 1, 3, 2, 8, 3), (2, 0, 1, 1, 0, 1), (2, 1, 6, 7, 64, 4)] if plane != BIG else [(3, 1, 3, 2, 8, 3)]
    for F, key, levels, search, smooth, C in cases:
        _chain(_video(F, H, W, C), _disc(H, W), key, levels, search, smooth, (plane, F, key, levels, search, smooth))


@pytest.mark.parametrize("frames,key", [(1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2), (7, 0), (7, 3), (7, 6)])
def test_every_frame_count_and_key_position(frames, key):
    H, W = 23, 33
    images, mask = _video(frames, H, W), _soft(H, W, 1)
    want = _chain(images, mask, key, 3, 2, 8, (frames, key))
    _same_bits(want[key], ref.binarise(mask).astype(np.float32), "the key frame is the binarised mask")
    per_frame = np.zeros((frames, H, W), np.float32)
    per_frame[key] = mask                                             # [F, H, W]: the key frame's mask is the one that is read
    got = propagate.propagate_masks(_dev(images), _dev(per_frame), key, 3, 2, 8)
    _same_bits(got.cpu().numpy(), want, "a mask per frame")
    got = propagate.propagate_masks(_dev(images), _dev(mask[None]), key, 3, 2, 8)
    _same_bits(got.cpu().numpy(), want, "[1, H, W]")


@pytest.mark.parametrize("mask", list(MASKS))
def test_the_chain_for_every_mask_and_image_form(mask):
    H, W = 16, 17
    for video in VIDEOS:
        m = MASKS[mask](H, W)
        want = _chain(VIDEOS[video](3, H, W, 3), m, 1, 3, 2, 8, (mask, video))
        if mask == "empty":
            assert (_bits(want) == 0).all()
        if mask == "full":
            assert (_bits(want) == ONE).all()
        if video == "constant":
            _same_bits(want, np.repeat(ref.binarise(m).astype(np.float32)[None], 3, axis=0), "equal frames: the binarised key mask")


def test_one_frame_per_chunk_gives_the_bits_of_one_chunk(monkeypatch):
    H, W = 40, 70
    images, mask = _video(5, H, W), _disc(H, W)
    t, m = _dev(images), _dev(mask)
    whole = propagate.propagate_masks(t, m, 2, 3, 2, 8).cpu().numpy()
    _same_bits(whole, ref.propagate_ref(images, mask, 2, 3, 2, 8), "one chunk")
    per_frame = _cabi.prop_pyramid_ws_bytes(1, H, W, 3)
    for frames in (1, 2):
        monkeypatch.setattr(propagate, "WS_CAP_BYTES", frames * per_frame + 8)
        _same_bits(propagate.propagate_masks(t, m, 2, 3, 2, 8).cpu().numpy(), whole, frames)
    _same_bits(propagate.propagate_masks(t.half(), m.half(), 2, 3, 2, 8).cpu().numpy(),
               ref.propagate_ref(t.half().float().cpu().numpy(), m.half().float().cpu().numpy(), 2, 3, 2, 8), "fp16 in chunks")
    for bad in (dict(key_frame=5), dict(key_frame=-1)):
        with pytest.raises(ValueError):
            propagate.propagate_masks(t, m, **bad)
    for bad_mask in (m[:-1], m[None].repeat(2, 1, 1), m[None, None]):
        with pytest.raises(ValueError):
            propagate.propagate_masks(t, bad_mask)
    with pytest.raises(ValueError):
        propagate.propagate_masks(t[0], m)


def test_node_returns_what_the_module_returns_on_the_inputs_device():
    H, W = 23, 33
    images, mask = _video(4, H, W), _disc(H, W)
    node = propagate_nodes.LanPaint_VideoMaskPropagate()
    want = ref.propagate_ref(images, mask, 1, 3, 2, 8)
    out, = node.propagate(torch.from_numpy(images), torch.from_numpy(mask), 1, 3, 2, 8)
    assert not out.is_cuda and out.dtype == torch.float32
    _same_bits(out.numpy(), want, "host in, host out")
    on_i, on_m = _dev(images), _dev(mask)
    out, = node.propagate(on_i, on_m, 1, 3, 2, 8)
    assert out.device == on_m.device and torch.equal(out, propagate.propagate_masks(on_i, on_m, 1, 3, 2, 8))
    out, = node.propagate(torch.from_numpy(images), torch.from_numpy(mask))       # the defaults: key 0, levels 4, search 2, smooth 8
    _same_bits(out.numpy(), ref.propagate_ref(images, mask), "defaults")
