"""The video temporal smooth on the MI355X (lanpaint_amd.temporal_smooth, csrc/temporal_smooth_kernel.hip) against the numpy
restatement tests/temporal_smooth_ref.py.  Integer arithmetic decides where a sample is taken and whether it counts, and the sums
are fp32 in a fixed order, so the device must give the restatement's values whatever tile or chunk a launch uses: every
comparison covers every element and has no tolerance.  NaN matches NaN, everything else matches by its bits.  The launch is
compared on its own, fed with the restatement's or with hand-made fields, and the whole call as well."""
import functools

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, temporal_smooth as ts, temporal_smooth_nodes
from tests import propagate_ref as ref
from tests import temporal_fill_ref as tref
from tests import temporal_smooth_ref as sref
from tests.compare import _same_ints as _same, _same_values
from tests.device import _dev
from tests.inputs import ALL_PLANES, THIN_PLANES, _random_masks, _rng, _video, _wild_video, plane_ids
from tests.motion_checks import _check_smooth as _check
from tests.temporal_clips import (RADII, check_smooth_ghost as check_ghost, check_smooth_noise as check_noise,
                                  check_smooth_pan as check_pan, ghost_clip, noise_clip, smooth_pan_clip as pan_clip)

pytestmark = pytest.mark.gpu
F, LEVELS = 5, 3


# ---- the launch alone ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene(H, W, channels=3, wild=False, one_mask=False):
    """(images, mask, known, fwd, bwd): a clip with the restatement's fields of it."""
    images = (_wild_video if wild else _video)(F, H, W, channels)
    mask = _random_masks(1 if one_mask else F, H, W)
    known = tref.known_bits(mask, F)
    return (images, mask, known, *sref.fields(images, known, "background", LEVELS, 2, 8))


def _launch(images, known, fwd, bwd, radius, tolerance, **kw):
    """Rows 0 .. F - 2 of fwd and 1 .. F - 1 of bwd are what a clip has."""
    n = images.shape[0]
    return ts.smooth_frames(_dev(fwd[:n - 1].astype(np.int32)) if n > 1 else None, _dev(bwd[1:].astype(np.int32)) if n > 1 else None,
                            _dev(known), _dev(images), radius, tolerance, **kw)


@pytest.mark.parametrize("channels", [1, 2, 3, 4])
@pytest.mark.parametrize("plane", ALL_PLANES, ids=plane_ids)
def test_the_launch_equals_the_restatement_on_every_plane(plane, channels):
    images, mask, known, fwd, bwd = _scene(*plane, channels)
    for radius in (1, 2, 8):                                           # 8 > F: every chain runs off the clip
        for tolerance in (0, 24, 255):
            want = sref.smooth_frames(images, known, fwd, bwd, radius, tolerance)
            _check(_launch(images, known, fwd, bwd, radius, tolerance), want, (plane, channels, radius, tolerance))
    if plane == (40, 70):
        support = sref.smooth_frames(images, known, fwd, bwd, 2, 24)[1]
        assert {0, 1, 2, 3, 4} <= set(np.unique(support).tolist())     # chains of every length, and rejected ones


@pytest.mark.parametrize("plane", THIN_PLANES, ids=plane_ids)
def test_the_launch_on_a_grid_one_block_wide(plane):
    images, mask, known, fwd, bwd = _scene(*plane)
    assert np.count_nonzero(fwd) >= 16 and np.count_nonzero(bwd) >= 16          # fields that move
    for radius, tolerance in ((1, 255), (2, 24), (8, 255)):
        want = sref.smooth_frames(images, known, fwd, bwd, radius, tolerance)
        assert tolerance < 255 or (want[1] > 0).sum() >= 16            # masked pixels whose walks stay inside the plane
        _check(_launch(images, known, fwd, bwd, radius, tolerance), want, (plane, radius, tolerance))


@pytest.mark.parametrize("channels", [6, 9])
def test_more_than_four_channels(channels):
    images, mask, known, fwd, bwd = _scene(23, 33, channels)
    for radius, tolerance in ((1, 255), (2, 24), (8, 60)):
        want = sref.smooth_frames(images, known, fwd, bwd, radius, tolerance)
        _check(_launch(images, known, fwd, bwd, radius, tolerance), want, (channels, radius, tolerance))
        assert (want[1] > 0).any()


def test_a_wild_video_with_nan_and_infinities():
    for plane in ((23, 33), (40, 70)):
        images, mask, known, fwd, bwd = _scene(*plane, wild=True)
        for radius, tolerance in ((2, 24), (2, 255), (8, 0)):
            want = sref.smooth_frames(images, known, fwd, bwd, radius, tolerance)
            _check(_launch(images, known, fwd, bwd, radius, tolerance), want, ("wild", plane, radius, tolerance))
    assert np.isnan(want[0]).any() and np.isinf(want[0]).any()


def test_a_mask_of_one_frame_one_frame_and_a_part_of_the_clip():
    images, mask, known, fwd, bwd = _scene(23, 33, one_mask=True)
    want = sref.smooth_frames(images, known, fwd, bwd, 2, 24)
    _check(_launch(images, known, fwd, bwd, 2, 24), want, "one mask")
    one = sref.smooth_frames(images[:1], known[:1], fwd[:1], bwd[:1], 2, 24)
    _check(_launch(images[:1], known[:1], fwd[:1], bwd[:1], 2, 24), one, "one frame, no fields")
    assert (one[0].view(np.uint32) == images[:1].view(np.uint32)).all()
    # frames 2 and 3 alone, with exactly the rows they read (radius 2: fwd of 2 .. 3, bwd of 1 .. 3); the rest is left as it was
    out = torch.full((F, 23, 33, 3), 7.0, device=_dev(mask).device)
    support = torch.full((F, 23, 33), 77, dtype=torch.int32, device=out.device)
    ts.smooth_frames(_dev(fwd[2:4].astype(np.int32)), _dev(bwd[1:4].astype(np.int32)), _dev(known[2:4]), _dev(images), 2, 24, first=2, count=2,
                     fwd_first=2, bwd_first=1, out=out, support=support)
    _same_values(out[2:4].cpu().numpy(), want[0][2:4], "a part: out")
    _same(support[2:4].cpu().numpy(), want[1][2:4], "a part: support")
    assert (out[[0, 1, 4]] == 7.0).all() and (support[[0, 1, 4]] == 77).all()
    with pytest.raises(ValueError):                                    # a row short
        ts.smooth_frames(_dev(fwd[2:3].astype(np.int32)), _dev(bwd[1:4].astype(np.int32)), _dev(known[2:4]), _dev(images), 2, 24, first=2,
                         count=2, fwd_first=2, bwd_first=1)


@pytest.mark.parametrize("plane", [(9, 15), (23, 33), (70, 130)], ids=plane_ids)
def test_hand_made_fields_of_several_pixels_with_odd_fractions(plane):
    H, W = plane
    rng = _rng(H, W, 9)
    images, known = _video(F, H, W, 3), tref.known_bits(_random_masks(F, H, W, 1, 0.6), F)
    gh, gw = ref.grid_of(H, W)
    fwd, bwd = (rng.integers(-75, 76, (F, gh, gw, 2)).astype(np.int64) for _ in range(2))     # up to 4 11/16 pixels
    want = sref.smooth_frames(images, known, fwd, bwd, 3, 255)
    _check(_launch(images, known, fwd, bwd, 3, 255), want, (plane, "hand-made"))
    q = ref.key_positions(H, W) + ref.pixel_vectors(fwd[0], H, W)
    under = known[0] == 0
    inside = (q[..., 0] >= 0) & (q[..., 0] <= 16 * (H - 1)) & (q[..., 1] >= 0) & (q[..., 1] <= 16 * (W - 1))
    assert (under & ~inside).any() and (under & inside & ((q & 15) != 0).all(axis=-1)).any()   # positions leave; fractional taps on both axes
    assert len(np.unique(want[1])) >= 5
    want = sref.smooth_frames(images, known, fwd, bwd, 2, 40)
    _check(_launch(images, known, fwd, bwd, 2, 40), want, (plane, "hand-made, tolerance 40"))


@pytest.mark.parametrize("channels", [1, 2, 3, 4, 6])
def test_tiles_with_nothing_masked_are_copied_whole(channels):
    """A small box under the mask: most waves (two rows of a 32 x 32 tile) hold no masked pixel and take the wave's copy, with
    rows that are and are not multiples of 16 bytes, full and cut tiles, and a frame with no mask at all."""
    for H, W in ((70, 130), (33, 64), (40, 72)):
        rng = _rng(H, W, channels, 11)
        images = _wild_video(F, H, W, channels)
        mask = np.zeros((F, H, W), np.float32)
        mask[:4, 30:36, 60:70] = 1                                     # the last frame has none
        known = tref.known_bits(mask, F)
        gh, gw = ref.grid_of(H, W)
        fwd, bwd = (rng.integers(-40, 41, (F, gh, gw, 2)).astype(np.int64) for _ in range(2))
        want = sref.smooth_frames(images, known, fwd, bwd, 2, 255)
        _check(_launch(images, known, fwd, bwd, 2, 255), want, ((H, W), channels))
        assert (want[1] > 0).any()


# ---- the whole call --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(H, W, motion):
    images, mask = _video(F, H, W, 3), _random_masks(F, H, W)
    return images, mask, sref.temporal_smooth_ref(images, mask, 2, 24, motion, LEVELS, 2, 8)


@pytest.mark.parametrize("motion", sref.MOTIONS)
@pytest.mark.parametrize("plane", [(23, 33), (70, 130)], ids=plane_ids)
def test_the_call_equals_the_restatement(plane, motion):
    images, mask, want = _reference(*plane, motion)
    _check(ts.temporal_smooth(_dev(images), _dev(mask), 2, 24, motion, LEVELS, 2, 8), want, (plane, motion))
    assert (want[1] > 0).any() and (want[0] != images).any()


def test_a_second_call_and_chunks_under_a_lowered_cap_give_the_same_bits(monkeypatch):
    H, W = 40, 70
    t, m = _dev(_video(9, H, W, 3)), _dev(_random_masks(9, H, W))
    stride = _cabi.prop_pyramid_ws_bytes(1, H, W, LEVELS)
    gh, gw = _cabi.prop_grid(H, W)
    for motion, planes in (("background", 2), ("picture", 3)):
        whole = ts.temporal_smooth(t, m, 2, 24, motion, LEVELS, 2, 8)
        again = ts.temporal_smooth(t, m, 2, 24, motion, LEVELS, 2, 8)
        per_frame = planes * stride + 2 * gh * gw * 8
        for frames in (1, 2, 4):                                       # 9 frames: nine chunks, 4 x 2 + 1, 2 x 4 + 1
            monkeypatch.setattr(ts, "WS_CAP_BYTES", (2 * 2 + frames) * per_frame + 8)
            chunked = ts.temporal_smooth(t, m, 2, 24, motion, LEVELS, 2, 8)
            for name, a, b, c in zip(("out", "support"), whole, again, chunked):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (motion, name, "a second call")
                assert torch.equal(a.view(torch.int32), c.view(torch.int32)), (motion, name, frames, "frames a chunk")
        monkeypatch.undo()


# ---- what follows from the rule, on the device ---------------------------------------------------------------------------------------------
def _run(clip, mask, *args):
    return [o.cpu().numpy() for o in ts.temporal_smooth(_dev(clip), _dev(mask), *args)]


@pytest.mark.parametrize("motion", sref.MOTIONS)
@pytest.mark.parametrize("radius", RADII)
def test_pan_with_alternating_flicker_is_recovered_bit_for_bit(radius, motion):
    _, clip, mask = pan_clip()
    check_pan(radius, motion, *_run(clip, mask, radius, 24, motion))


@pytest.mark.parametrize("radius", RADII)
def test_noise_variance_falls_as_the_weights_say(radius):
    _, clip, mask = noise_clip()
    check_noise(radius, *_run(clip, mask, radius, 24))


def test_an_object_beyond_the_tolerance_leaves_no_ghost_and_an_empty_mask_the_images():
    clip, mask = ghost_clip()
    check_ghost(*_run(clip, mask, 2, 24))
    out, support = _run(clip, np.zeros_like(mask), 2, 24)
    assert (out.view(np.uint32) == clip.view(np.uint32)).all() and (support == -1).all()


def test_node_returns_what_the_module_returns_on_the_inputs_device():
    images, mask, want = _reference(23, 33, "picture")
    node = temporal_smooth_nodes.LanPaint_VideoTemporalSmooth()
    image, share = node.smooth(torch.from_numpy(images), torch.from_numpy(mask), 2, 24, "picture", LEVELS, 2, 8)
    assert not image.is_cuda and not share.is_cuda
    _same_values(image.numpy(), want[0], "host in, host out")
    _same_values(share.numpy(), (np.maximum(want[1], 0) / np.float32(4)).astype(np.float32), "support / (2 radius), 0 outside the mask")
    on_i, on_m = _dev(images), _dev(mask)
    image, share = node.smooth(on_i, on_m, 2, 24, "picture", LEVELS, 2, 8)
    direct = ts.temporal_smooth(on_i, on_m, 2, 24, "picture", LEVELS, 2, 8)
    assert image.device == on_i.device and share.device == on_m.device and torch.equal(image.view(torch.int32), direct[0].view(torch.int32))
    image, _ = node.smooth(torch.from_numpy(images), torch.from_numpy(mask))    # the defaults: radius 2, tolerance 24, background, 4, 2, 8
    _same_values(image.numpy(), sref.temporal_smooth_ref(images, mask)[0], "defaults")
