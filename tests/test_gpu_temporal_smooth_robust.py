"""The robust video temporal smooth on the MI355X (lanpaint_amd.temporal_smooth_robust, csrc/temporal_smooth_kernel.hip) against the
numpy restatement tests/temporal_smooth_robust_ref.py.  Integer arithmetic decides where a sample is taken, which sample is the
reference and what counts, and the sums are fp32 in a fixed order, so the device must give the restatement's values whatever
tile or chunk a launch uses: every comparison covers every element and has no tolerance.  NaN matches NaN, everything else matches
by its bits.  A test on random content first asserts, on the restatement alone, that every branch of the rule occurs in it
(`rref.ALL_BRANCHES`); the seeds, radii and tolerances were chosen on the CPU so that it does.  Planes of fewer than 23 x 33 pixels
cannot hold every branch and are compared all the same; at radius 2 the border cannot cut a chain behind a rejected sample."""
import functools

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, shots, temporal_smooth as ts, temporal_smooth_robust as tr, temporal_smooth_robust_nodes
from tests import propagate_ref as ref
from tests import temporal_fill_ref as tref
from tests import temporal_smooth_ref as sref
from tests import temporal_smooth_robust_ref as rref
from tests.compare import _same_ints as _same, _same_values
from tests.device import _dev
from tests.inputs import ALL_PLANES, THIN_PLANES, _random_masks, _rng, _video, _wild_video, plane_ids
from tests.motion_checks import _check_robust_smooth as _check
from tests.temporal_clips import (RADII, check_ghost_removed, check_pan_equals_plain, check_pop, check_robust_noise as check_noise,
                                  check_two_frame_pop, ghost_clip, noise_clip, pop_clip, smooth_pan_clip as pan_clip)

pytestmark = pytest.mark.gpu
F, LEVELS = 5, 3
NAMES = ("out", "support", "replaced")


def _popped(images, seed, share=0.12):
    """A share of the pixels of every frame moved by +-0.3 in every channel: outliers for a median to find."""
    rng = _rng(*images.shape, seed, 21)
    pick = rng.random(images.shape[:3]) < share
    images = images.copy()
    images[pick] += rng.choice(np.float32([-0.3, 0.3]), (int(pick.sum()), 1))
    return images


class _Wants:
    """The restatement's results of a test's runs, and the branches they took together."""

    def __init__(self):
        self.runs, self.seen = [], set()

    def add(self, what, images, known, fwd, bwd, radius, tolerance, **kw):
        trace = {}
        want = rref.robust_frames(images, known, fwd, bwd, radius, tolerance, trace=trace)
        self.seen |= rref.branches(trace, radius, images.shape[0])
        self.runs.append((what, images, known, fwd, bwd, radius, tolerance, kw, want))
        return want

    def every_branch(self):
        assert rref.ALL_BRANCHES <= self.seen, sorted(rref.ALL_BRANCHES - self.seen)

    def compare(self):
        for what, images, known, fwd, bwd, radius, tolerance, kw, want in self.runs:
            _check(_launch(images, known, fwd, bwd, radius, tolerance, **kw), want, what)


# ---- the launch alone ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene(H, W, channels=3, wild=False, one_mask=False):
    """(images, mask, known, fwd, bwd): a clip with outliers in it and the restatement's fields of it."""
    images = _wild_video(F, H, W, channels) if wild else _popped(_video(F, H, W, channels), 1)
    mask = _random_masks(1 if one_mask else F, H, W)
    known = tref.known_bits(mask, F)
    return (images, mask, known, *sref.fields(images, known, "background", LEVELS, 2, 8))


def _launch(images, known, fwd, bwd, radius, tolerance, **kw):
    """Rows 0 .. F - 2 of fwd and 1 .. F - 1 of bwd are what a clip has."""
    n = images.shape[0]
    return tr.robust_frames(_dev(fwd[:n - 1].astype(np.int32)) if n > 1 else None, _dev(bwd[1:].astype(np.int32)) if n > 1 else None,
                            _dev(known), _dev(images), radius, tolerance, **kw)


@pytest.mark.parametrize("channels", [1, 2, 3, 4])
@pytest.mark.parametrize("plane", ALL_PLANES, ids=plane_ids)
def test_the_launch_equals_the_restatement_on_every_plane(plane, channels):
    images, mask, known, fwd, bwd = _scene(*plane, channels)
    wants = _Wants()
    for radius in (1, 2, 8):                                           # 8 > F: every chain runs off the clip
        for tolerance in (0, 24, 255):
            wants.add((plane, channels, radius, tolerance), images, known, fwd, bwd, radius, tolerance)
    if plane[0] * plane[1] >= 23 * 33:
        wants.every_branch()
    wants.compare()


@pytest.mark.parametrize("plane", THIN_PLANES, ids=plane_ids)
def test_the_launch_on_a_grid_one_block_wide(plane):
    images, mask, known, fwd, bwd = _scene(*plane)
    assert np.count_nonzero(fwd) >= 16 and np.count_nonzero(bwd) >= 16          # fields that move
    wants = _Wants()
    for radius, tolerance in ((1, 255), (2, 24), (8, 255)):
        want = wants.add((plane, radius, tolerance), images, known, fwd, bwd, radius, tolerance)
        assert tolerance < 255 or (want[1] > 0).sum() >= 16            # masked pixels whose walks stay inside the plane
    wants.compare()


@pytest.mark.parametrize("channels", [6, 9])
def test_more_than_four_channels(channels):
    images, mask, known, fwd, bwd = _scene(23, 33, channels)
    wants = _Wants()
    for radius, tolerance in ((1, 255), (2, 24), (8, 60)):
        want = wants.add((channels, radius, tolerance), images, known, fwd, bwd, radius, tolerance)
        assert (want[1] > 0).any()
    wants.every_branch()
    wants.compare()


@pytest.mark.parametrize("plane", [(23, 33), (70, 130)], ids=plane_ids)
def test_eighteen_frames_with_hand_made_fields_rank_seventeen_values(plane):
    """R = 8 in a clip of 18 frames: the frames 8 and 9 have all 17 samples, and fields of up to 4 11/16 pixels make chains leave
    the plane at every length."""
    H, W = plane
    frames = 18
    rng = _rng(H, W, 18)
    images = _popped(_video(frames, H, W, 3), 2, 0.3)
    known = tref.known_bits(_random_masks(frames, H, W, 1, 0.5), frames)
    gh, gw = ref.grid_of(H, W)
    fwd, bwd = (rng.integers(-75, 76, (frames, gh, gw, 2)).astype(np.int64) for _ in range(2))
    wants = _Wants()
    trace = {}
    rref.robust_frames(images, known, fwd, bwd, 8, 40, frames=(8, 9), trace=trace)
    counts = np.concatenate([trace[t][2].sum(axis=1) for t in (8, 9)])
    assert (counts == 17).any() and len(np.unique(counts)) >= 8        # the full rank, and chains that leave at many lengths
    for radius, tolerance in ((8, 40), (8, 255), (3, 60)):
        wants.add((plane, "hand-made", radius, tolerance), images, known, fwd, bwd, radius, tolerance)
    wants.every_branch()
    wants.compare()


def test_a_palette_of_four_values_where_the_tie_order_decides():
    """Every pixel is one of four greys, so most lumas along a walk are equal and j* is whichever the walk's order puts at the
    median's place."""
    H, W = 23, 33
    rng = _rng(H, W, 4)
    palette = np.float32([0.1, 0.35, 0.6, 0.85])
    images = np.repeat(palette[rng.integers(0, 4, (F, H, W, 1))], 3, axis=-1)                    # grey: four lumas in all
    known = tref.known_bits(_random_masks(F, H, W, 2, 0.6), F)
    gh, gw = ref.grid_of(H, W)
    # one vector of whole pixels per frame: every sample is a pixel of the palette
    fwd, bwd = (np.broadcast_to(16 * rng.integers(-2, 3, (F, 1, 1, 2)), (F, gh, gw, 2)).astype(np.int64) for _ in range(2))
    wants = _Wants()
    trace = {}
    rref.robust_frames(images, known, fwd, bwd, 2, 70, trace=trace)
    tied = 0
    for t, (ys, xs, exists, js, accepted, case) in trace.items():
        s = rref.walk(images, known, fwd, bwd, 2, t)[3]
        Y = np.where(exists, rref.luma_of(s), -1)
        tied += int(((Y == Y[np.arange(len(js)), js][:, None]).sum(axis=1) >= 2).sum())
    print("pixels whose median luma is shared:", tied)
    assert tied >= 1000                                                 # the median's luma is shared: the order index decided
    for radius, tolerance in ((2, 70), (2, 0), (1, 70), (8, 130)):
        wants.add(("palette", radius, tolerance), images, known, fwd, bwd, radius, tolerance)
    wants.every_branch()
    wants.compare()


def test_a_wild_video_with_nan_and_infinities():
    wants = _Wants()
    for plane in ((23, 33), (40, 70)):
        images, mask, known, fwd, bwd = _scene(*plane, wild=True)
        for radius, tolerance in ((1, 100), (2, 24), (2, 255), (8, 0)):
            want = wants.add(("wild", plane, radius, tolerance), images, known, fwd, bwd, radius, tolerance)
    assert np.isnan(want[0]).any() and np.isinf(want[0]).any()
    wants.every_branch()
    wants.compare()


def test_a_mask_of_one_frame_one_and_two_frames_and_a_part_of_the_clip():
    images, mask, known, fwd, bwd = _scene(23, 33, one_mask=True)
    wants = _Wants()
    want = wants.add("one mask", images, known, fwd, bwd, 2, 24)
    wants.add("one mask, radius 1", images, known, fwd, bwd, 1, 24)
    wants.add("one mask, radius 3", images, known, fwd, bwd, 3, 24)  # the border can cut a chain behind its second step
    one = wants.add("one frame, no fields", images[:1], known[:1], fwd[:1], bwd[:1], 2, 24)
    assert (one[0].view(np.uint32) == images[:1].view(np.uint32)).all() and (one[2] <= 0).all()
    two = wants.add("two frames", images[:2], known[:2], fwd[:2], bwd[:2], 2, 24)
    plain = sref.smooth_frames(images[:2], known[:2], fwd[:2], bwd[:2], 2, 24)
    assert (two[0].view(np.uint32) == plain[0].view(np.uint32)).all() and (two[1] == plain[1]).all() and (two[2] <= 0).all()
    wants.every_branch()
    wants.compare()
    # frames 2 and 3 alone, with exactly the rows they read (radius 2: fwd of 2 .. 3, bwd of 1 .. 3); the rest is left as it was
    out = torch.full((F, 23, 33, 3), 7.0, device=_dev(mask).device)
    support = torch.full((F, 23, 33), 77, dtype=torch.int32, device=out.device)
    replaced = torch.full((F, 23, 33), 55, dtype=torch.int32, device=out.device)
    tr.robust_frames(_dev(fwd[2:4].astype(np.int32)), _dev(bwd[1:4].astype(np.int32)), _dev(known[2:4]), _dev(images), 2, 24, first=2, count=2,
                     fwd_first=2, bwd_first=1, out=out, support=support, replaced=replaced)
    _same_values(out[2:4].cpu().numpy(), want[0][2:4], "a part: out")
    _same(support[2:4].cpu().numpy(), want[1][2:4], "a part: support")
    _same(replaced[2:4].cpu().numpy(), want[2][2:4], "a part: replaced")
    assert (out[[0, 1, 4]] == 7.0).all() and (support[[0, 1, 4]] == 77).all() and (replaced[[0, 1, 4]] == 55).all()
    with pytest.raises(ValueError):                                    # a row short
        tr.robust_frames(_dev(fwd[2:3].astype(np.int32)), _dev(bwd[1:4].astype(np.int32)), _dev(known[2:4]), _dev(images), 2, 24, first=2,
                         count=2, fwd_first=2, bwd_first=1)


@pytest.mark.parametrize("channels", [1, 2, 3, 4, 6])
def test_tiles_with_nothing_masked_are_copied_whole(channels):
    """A small box under the mask: most waves (two rows of a 32 x 32 tile) hold no masked pixel and take the wave's copy, with
    rows that are and are not multiples of 16 bytes, full and cut tiles, and a frame with no mask at all.  The three planes
    together hold every branch of the rule."""
    wants = _Wants()
    for H, W in ((70, 130), (33, 64), (40, 72)):
        rng = _rng(H, W, channels, 11)
        images = _wild_video(F, H, W, channels)
        mask = np.zeros((F, H, W), np.float32)
        mask[:4, 30:36, 60:70] = 1                                     # the last frame has none
        known = tref.known_bits(mask, F)
        gh, gw = ref.grid_of(H, W)
        fwd, bwd = (rng.integers(-40, 41, (F, gh, gw, 2)).astype(np.int64) for _ in range(2))
        for radius, tolerance in ((2, 255), (1, 100), (3, 100), (3, 160)):
            want = wants.add(((H, W), channels, radius, tolerance), images, known, fwd, bwd, radius, tolerance)
            assert (want[1] > 0).any() and (want[2][4] == -1).all()
    wants.every_branch()
    wants.compare()


# ---- the whole call --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(H, W, motion):
    images, mask = _popped(_video(F, H, W, 3), 3), _random_masks(F, H, W)
    trace = {}
    want = rref.temporal_smooth_robust_ref(images, mask, 2, 24, motion, LEVELS, 2, 8, trace=trace)
    return images, mask, want, rref.branches(trace, 2, F)


AT_RADIUS_TWO = rref.ALL_BRANCHES - {"a chain cut by the border with an accepted sample behind a rejected one"}


@pytest.mark.parametrize("motion", sref.MOTIONS)
@pytest.mark.parametrize("plane", [(23, 33), (70, 130)], ids=plane_ids)
def test_the_call_equals_the_restatement(plane, motion):
    images, mask, want, seen = _reference(*plane, motion)
    # at radius 2 a chain with an accepted sample behind a rejected one has both its steps: the border cannot have cut it
    assert AT_RADIUS_TWO <= seen, sorted(AT_RADIUS_TWO - seen)
    assert (want[1] > 0).any() and (want[0] != images).any() and (want[2] == 1).any()
    _check(tr.temporal_smooth_robust(_dev(images), _dev(mask), 2, 24, motion, LEVELS, 2, 8), want, (plane, motion))


def test_a_second_call_and_chunks_under_a_lowered_cap_give_the_same_bits(monkeypatch):
    H, W = 40, 70
    t, m = _dev(_popped(_video(9, H, W, 3), 4)), _dev(_random_masks(9, H, W))
    stride = _cabi.prop_pyramid_ws_bytes(1, H, W, LEVELS)
    gh, gw = _cabi.prop_grid(H, W)
    for motion, planes in (("background", 2), ("picture", 3)):
        whole = tr.temporal_smooth_robust(t, m, 2, 24, motion, LEVELS, 2, 8)
        again = tr.temporal_smooth_robust(t, m, 2, 24, motion, LEVELS, 2, 8)
        assert (whole[2] == 1).any()
        per_frame = planes * stride + 2 * gh * gw * 8
        for frames in (1, 2, 4):                                       # 9 frames: nine chunks, 4 x 2 + 1, 2 x 4 + 1
            monkeypatch.setattr(ts, "WS_CAP_BYTES", (2 * 2 + frames) * per_frame + 8)
            chunked = tr.temporal_smooth_robust(t, m, 2, 24, motion, LEVELS, 2, 8)
            for name, a, b, c in zip(NAMES, whole, again, chunked):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (motion, name, "a second call")
                assert torch.equal(a.view(torch.int32), c.view(torch.int32)), (motion, name, frames, "frames a chunk")
        monkeypatch.undo()


# ---- what follows from the rule, on the device ---------------------------------------------------------------------------------------------
def _run(clip, mask, *args):
    return [o.cpu().numpy() for o in tr.temporal_smooth_robust(_dev(clip), _dev(mask), *args)]


def _plain(clip, mask, *args):
    return [o.cpu().numpy() for o in ts.temporal_smooth(_dev(clip), _dev(mask), *args)]


@pytest.mark.parametrize("radius", RADII)
def test_pan_with_flicker_gives_the_plain_rules_bits(radius):
    _, clip, mask = pan_clip()
    check_pan_equals_plain(_run(clip, mask, radius, 24), _plain(clip, mask, radius, 24))


@pytest.mark.parametrize("radius", RADII)
def test_a_pop_of_one_frame_is_removed_and_the_plain_rule_keeps_it(radius):
    clip, mask = pop_clip((3,))
    check_pop(_run(clip, mask, radius, 24), _plain(clip, mask, radius, 24))


@pytest.mark.parametrize("radius", RADII)
def test_a_pop_of_two_frames_is_removed_from_radius_two_on(radius):
    clip, mask = pop_clip((3, 4))
    check_two_frame_pop(radius, _run(clip, mask, radius, 24))


def test_the_ghost_is_removed_an_empty_mask_returns_the_images_and_noise_falls_as_the_weights_say():
    clip, mask = ghost_clip()
    check_ghost_removed(_run(clip, mask, 2, 24))
    out, support, replaced = _run(clip, np.zeros_like(mask), 2, 24)
    assert (out.view(np.uint32) == clip.view(np.uint32)).all() and (support == -1).all() and (replaced == -1).all()
    _, clip, mask = noise_clip()
    for radius in RADII:
        check_noise(radius, *_run(clip, mask, radius, 24))


# ---- the nodes -----------------------------------------------------------------------------------------------------------------------------
def test_nodes_return_what_the_module_returns_on_the_inputs_device():
    images, mask, want, seen = _reference(23, 33, "picture")
    assert AT_RADIUS_TWO <= seen, sorted(AT_RADIUS_TWO - seen)
    node = temporal_smooth_robust_nodes.LanPaint_VideoTemporalSmoothRobust()
    image, share, replaced = node.smooth(torch.from_numpy(images), torch.from_numpy(mask), 2, 24, "picture", LEVELS, 2, 8)
    assert not image.is_cuda and not share.is_cuda and not replaced.is_cuda
    _same_values(image.numpy(), want[0], "host in, host out")
    _same_values(share.numpy(), (np.maximum(want[1], 0) / np.float32(4)).astype(np.float32), "support / (2 radius), 0 outside the mask")
    _same_values(replaced.numpy(), np.maximum(want[2], 0).astype(np.float32), "replaced, 0 outside the mask")
    on_i, on_m = _dev(images), _dev(mask)
    image, share, replaced = node.smooth(on_i, on_m, 2, 24, "picture", LEVELS, 2, 8)
    direct = tr.temporal_smooth_robust(on_i, on_m, 2, 24, "picture", LEVELS, 2, 8)
    assert image.device == on_i.device and share.device == on_m.device and replaced.device == on_m.device
    assert torch.equal(image.view(torch.int32), direct[0].view(torch.int32))
    image, _, _ = node.smooth(torch.from_numpy(images), torch.from_numpy(mask))    # the defaults: radius 2, tolerance 24, background, 4, 2, 8
    _same_values(image.numpy(), rref.temporal_smooth_robust_ref(images, mask)[0], "defaults")
    # per shot: two ranges are two clips, and no shots are one
    ranges = [(0, 2), (2, F)]
    per_shot = temporal_smooth_robust_nodes.LanPaint_VideoTemporalSmoothRobustShots()
    got = per_shot.smooth(torch.from_numpy(images), torch.from_numpy(mask), 2, 24, "picture", LEVELS, 2, 8, shots=ranges)
    module = shots.temporal_smooth_robust_shots(on_i, on_m, ranges, 2, 24, "picture", LEVELS, 2, 8)
    for lo, hi in ranges:
        part = rref.temporal_smooth_robust_ref(images[lo:hi], mask[lo:hi], 2, 24, "picture", LEVELS, 2, 8)
        _same_values(got[0][lo:hi].numpy(), part[0], ("per shot: image", lo))
        _same_values(got[2][lo:hi].numpy(), np.maximum(part[2], 0).astype(np.float32), ("per shot: replaced", lo))
        _check([o[lo:hi].contiguous() for o in module], part, ("per shot: module", lo))
    whole = per_shot.smooth(on_i, on_m, 2, 24, "picture", LEVELS, 2, 8)
    assert all(torch.equal(a, b) for a, b in zip(whole, node.smooth(on_i, on_m, 2, 24, "picture", LEVELS, 2, 8)))
