"""The occlusion-aware video mask propagate on the MI355X (lanpaint_amd.propagate_visible, lp_prop_visible and lp_prop_occlude in
csrc/propagate_kernel.hip) against the numpy restatement tests/propagate_visible_ref.py.  The rule is integer arithmetic, so every
comparison covers every element and has no tolerance.  Each of the two launches is compared on its own, fed with inputs made here,
and the whole chain as well.  Without the feature this file fails at its imports."""
import functools

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, propagate, propagate_visible, propagate_visible_nodes
from tests import propagate_ref as ref
from tests import propagate_visible_ref as vref
from tests.compare import _same_bits, _same_ints as _same
from tests.device import DEV, _dev
from tests.helpers import record_launches
from tests.inputs import (VISIBLE_MASKS as MASKS, VISIBLE_PLANES as PLANES, _border_disc as _disc, _flags, _occluded_video, _positions,
                          _rng, _visible_lumas as _lumas)

pytestmark = pytest.mark.gpu


# ---- inputs of the two launches -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("positions", ["key", "smooth", "outside"])
@pytest.mark.parametrize("lumas", ["noisy", "dark"])
def test_visible_flags_equal_the_restatement(positions, lumas):
    seen = set()
    for H, W in PLANES:
        P = _positions(positions, H, W)
        Yt, Yk = _lumas(lumas, H, W)
        for name, make in MASKS.items():
            m = make(H, W)
            for occlusion in (1, 16, 255):
                want = vref.visible_flags(Yt, Yk, P, m, occlusion)
                got = propagate_visible.visible_flags(_dev(P.astype(np.int32)), _dev(Yt), _dev(Yk), _dev(m), occlusion)
                assert got.dtype == torch.int32 and tuple(got.shape) == ref.grid_of(H, W)
                _same(got.cpu().numpy(), want, ("flags", (H, W), positions, lumas, name, occlusion))
                seen.update((name, int(v)) for v in np.unique(want))
                if name == "empty":
                    assert not want.any()
    assert {("full", 0), ("full", 1), ("disc", 0), ("disc", 1), ("sparse", 0), ("sparse", 1)} <= seen


def test_visible_flags_on_unaligned_planes_take_the_scalar_path_with_the_same_bits():
    """A width that is a multiple of 4 but planes that do not start on 16 bytes: views one element into a larger buffer."""
    H, W = 33, 64
    P, (Yt, Yk), m = _positions("smooth", H, W), _lumas("noisy", H, W), _disc(H, W)
    want = vref.visible_flags(Yt, Yk, P, m, 16)

    def shifted(a):
        buf = torch.empty(a.size + 1, dtype=torch.from_numpy(a[:0]).dtype, device=DEV)
        view = buf[1:].view(a.shape)
        view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        return view
    got = propagate_visible.visible_flags(shifted(P.astype(np.int32)), shifted(Yt), _dev(Yk), shifted(m), 16)
    _same(got.cpu().numpy(), want, "unaligned")
    c = _rng(H, W, 12).integers(0, 257, (H, W))
    out, hidden, _ = propagate_visible.occlude(shifted((c / 256).astype(np.float32)), _dev(want.astype(np.int32)), 3)
    cv = vref.occlude(c, want)
    _same_bits(out.cpu().numpy(), cv.astype(np.float32) / np.float32(256), "unaligned mask")
    _same_bits(hidden.cpu().numpy(), (c - cv).astype(np.float32) / np.float32(256), "unaligned hidden")


@pytest.mark.parametrize("kind", ["none", "all", "checkerboard", "random"])
def test_occlude_equals_the_restatement(kind):
    for H, W in PLANES:
        flags = _flags(kind, *ref.grid_of(H, W))
        c = _rng(H, W, 12).integers(0, 257, (H, W))
        c[_rng(H, W, 13).random((H, W)) < 0.3] = 256
        cv = vref.occlude(c, flags)
        assert (cv <= c).all() and (kind != "none" or (cv == c).all()) and (kind != "all" or not cv.any())
        for levels in (1, 4, 6):
            out, hidden, mpyr = propagate_visible.occlude(_dev((c / 256).astype(np.float32)), _dev(flags.astype(np.int32)), levels)
            _same_bits(out.cpu().numpy(), cv.astype(np.float32) / np.float32(256), ("mask", (H, W), kind))
            _same_bits(hidden.cpu().numpy(), (c - cv).astype(np.float32) / np.float32(256), ("hidden", (H, W), kind))
            want = ref.pyramid((cv >= 128).astype(np.uint8), levels, ref.down_mask)
            host = mpyr.cpu()
            for lv in range(levels):
                _same(propagate.level_view(host, H, W, lv).numpy()[0], want[lv], ("next bits", (H, W), kind, levels, lv))


# ---- the whole chain ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _want(F, H, W, key, occlusion):
    images, mask = _occluded_video(F, H, W)
    trace = {}
    return vref.propagate_visible_ref(images, mask, key, 3, 2, 8, occlusion, trace), trace


@pytest.mark.parametrize("plane", [(23, 33), (70, 130)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("frames,key", [(1, 0), (2, 1), (3, 1), (7, 3)])
def test_the_chain_with_an_occluder_equals_the_restatement_bit_for_bit(plane, frames, key):
    H, W = plane
    images, mask = _occluded_video(frames, H, W)
    (want, want_hidden), trace = _want(frames, H, W, key, 16)
    got, hidden = propagate_visible.propagate_masks_visible(_dev(images), _dev(mask), key, 3, 2, 8)     # the default occlusion
    assert got.is_cuda and hidden.is_cuda and got.dtype == hidden.dtype == torch.float32
    _same_bits(got.cpu().numpy(), want, ("mask", plane, frames, key))
    _same_bits(hidden.cpu().numpy(), want_hidden, ("hidden", plane, frames, key))
    _same_bits(want[key], ref.binarise(mask).astype(np.float32), "the key frame is the binarised mask")
    assert not want_hidden[key].any()
    if frames == 7 and plane == (70, 130):                             # the occluder is seen, and not everything is taken for one
        flags = np.stack([trace[t][2] for t in trace])
        assert flags.any() and not flags.all() and want_hidden.sum() > 0 and want.sum() > 0


def test_the_chain_at_other_thresholds_and_mask_forms():
    H, W = 23, 33
    images, mask = _occluded_video(3, H, W)
    t, m = _dev(images), _dev(mask)
    for occlusion in (1, 255):
        want, want_hidden = _want(3, H, W, 1, occlusion)[0]
        got, hidden = propagate_visible.propagate_masks_visible(t, m, 1, 3, 2, 8, occlusion)
        _same_bits(got.cpu().numpy(), want, ("mask", occlusion))
        _same_bits(hidden.cpu().numpy(), want_hidden, ("hidden", occlusion))
    want, want_hidden = _want(3, H, W, 1, 16)[0]
    per_frame = np.zeros((3, H, W), np.float32)
    per_frame[1] = mask                                               # [F, H, W]: the key frame's mask is the one that is read
    for form in (_dev(per_frame), m[None]):
        got, hidden = propagate_visible.propagate_masks_visible(t, form, 1, 3, 2, 8, 16)
        _same_bits(got.cpu().numpy(), want, "mask forms")
        _same_bits(hidden.cpu().numpy(), want_hidden, "mask forms")
    empty, none = propagate_visible.propagate_masks_visible(t, torch.zeros_like(m), 1, 3, 2, 8, 1)
    assert not empty.any() and not none.any()
    still = t[:1].repeat(3, 1, 1, 1)
    got, hidden = propagate_visible.propagate_masks_visible(still, m, 0, 3, 2, 8, 1)
    _same_bits(got.cpu().numpy(), np.repeat(ref.binarise(mask).astype(np.float32)[None], 3, axis=0), "equal frames")
    assert not hidden.any()


def test_occlusion_zero_is_propagate_masks_and_makes_no_new_launch(monkeypatch):
    H, W = 40, 70
    images, mask = _occluded_video(4, H, W)
    t, m = _dev(images), _dev(mask)
    names = record_launches(monkeypatch, propagate_visible)           # this module's launches and the shared layer's: the pyramids
    want = propagate.propagate_masks(t, m, 2, 3, 2, 8)
    plain = list(names)
    assert set(plain) == {"lp_prop_luma"}
    del names[:]
    got, hidden = propagate_visible.propagate_masks_visible(t, m, 2, 3, 2, 8, 0)
    assert names == plain and torch.equal(got, want)                  # nothing but what propagate_masks launches itself
    assert hidden.is_cuda and hidden.dtype == torch.float32 and tuple(hidden.shape) == (4, H, W) and not hidden.any()
    del names[:]
    propagate_visible.propagate_masks_visible(t, m, 2, 3, 2, 8, 16)
    assert [n for n in names if n != "lp_prop_luma"] == ["lp_prop_visible", "lp_prop_occlude"] * 3    # two behind each of the three advances
    assert [n for n in names if n == "lp_prop_luma"] == plain


def test_one_frame_per_chunk_gives_the_bits_of_one_chunk(monkeypatch):
    """The chunks are propagate's (the new module reuses its chain_frames), so its cap is the one that is lowered; the key frame's
    luma has to outlive the chunk it came in."""
    H, W = 40, 70
    images, mask = _occluded_video(5, H, W)
    t, m = _dev(images), _dev(mask)
    whole, whole_hidden = (a.cpu().numpy() for a in propagate_visible.propagate_masks_visible(t, m, 2, 3, 2, 8, 16))
    want, want_hidden = _want(5, H, W, 2, 16)[0]
    _same_bits(whole, want, "one chunk")
    _same_bits(whole_hidden, want_hidden, "one chunk")
    per_frame = _cabi.prop_pyramid_ws_bytes(1, H, W, 3)
    for frames in (1, 2):
        monkeypatch.setattr(propagate_visible.propagate, "WS_CAP_BYTES", frames * per_frame + 8)
        got, hidden = propagate_visible.propagate_masks_visible(t, m, 2, 3, 2, 8, 16)
        _same_bits(got.cpu().numpy(), whole, frames)
        _same_bits(hidden.cpu().numpy(), whole_hidden, frames)
    for bad in (dict(key_frame=5), dict(key_frame=-1), dict(occlusion=256)):
        with pytest.raises(ValueError):
            propagate_visible.propagate_masks_visible(t, m, **bad)
    for bad_mask in (m[:-1], m[None].repeat(2, 1, 1), m[None, None]):
        with pytest.raises(ValueError):
            propagate_visible.propagate_masks_visible(t, bad_mask)


def test_node_returns_what_the_module_returns_on_the_inputs_device():
    H, W = 23, 33
    images, mask = _occluded_video(3, H, W)
    node = propagate_visible_nodes.LanPaint_VideoMaskPropagateVisible()
    want, want_hidden = _want(3, H, W, 1, 16)[0]
    out, hidden = node.propagate(torch.from_numpy(images), torch.from_numpy(mask), 1, 3, 2, 8, 16)
    assert not out.is_cuda and not hidden.is_cuda and out.dtype == hidden.dtype == torch.float32
    _same_bits(out.numpy(), want, "host in, host out")
    _same_bits(hidden.numpy(), want_hidden, "host in, host out")
    on_i, on_m = _dev(images), _dev(mask)
    out, hidden = node.propagate(on_i, on_m, 1, 3, 2, 8, 16)
    m, h = propagate_visible.propagate_masks_visible(on_i, on_m, 1, 3, 2, 8, 16)
    assert out.device == hidden.device == on_m.device and torch.equal(out, m) and torch.equal(hidden, h)
    out, hidden = node.propagate(on_i, on_m)                          # the defaults: key 0, levels 4, search 2, smooth 8, occlusion 16
    m, h = propagate_visible.propagate_masks_visible(on_i, on_m, 0, 4, 2, 8, 16)
    assert torch.equal(out, m) and torch.equal(hidden, h)
