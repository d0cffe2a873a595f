"""The long clips of tests/temporal_clips.py under the three restatements alone (tests/temporal_fill_ref.py,
tests/temporal_fill_checked_ref.py, tests/temporal_smooth_ref.py): no device.  tests/test_gpu_temporal_long_clips.py compares the
kernels with these results, and that says something about origins tens of frames old, about `reach` at and one below an age that
occurs, about disputes on a long clip and about smooth chains of 8 steps only if the clips make the rule go there.  That they do is
asserted here as conditions; the counts seen when this was written stand beside them in brackets.  The cases and their cached
restatement results are shared with the device's tests."""

import numpy as np
import pytest

from tests import temporal_clips as clips
from tests import temporal_fill_checked_ref as cref
from tests import temporal_fill_ref as tref
from tests import temporal_smooth_ref as sref
from tests.compare import _f32_bits as _bits
from tests.temporal_clips import (LONG_ARRIVES as ARRIVES, LONG_CHANGE as CHANGE, LONG_FRAMES as FRAMES, LONG_LEAVES as LEAVES,
                                  LONG_LEVELS as LEVELS, LONG_PLANE as PLANE, LONG_SEARCH as SEARCH, LONG_SMOOTH as SMOOTH,
                                  LONG_SMOOTH_FRAMES as SMOOTH_FRAMES, long_checked_clip as checked_clip,
                                  long_checked_want as checked_want, long_fill_clip as fill_clip, long_fill_want as fill_want,
                                  long_smooth_clip as smooth_clip, long_smooth_want as smooth_want)


def same_bits(a, b):
    """Two results of a restatement: every output equal, NaN by its bits too."""
    return all(x.shape == y.shape and ((_bits(x) == _bits(y)).all() if x.dtype == np.float32 else (x == y).all()) for x, y in zip(a, b))


def ages(mask, source):
    """The ages |t - source| of the borrowed pixels: masked, with an origin."""
    m = (mask if mask.ndim == 3 else np.broadcast_to(mask, source.shape)) == 1
    return np.abs(np.arange(len(source))[:, None, None] - source)[m & (source >= 0)]


# ---- the plain fill ----------------------------------------------------------------------------------------------------------------------
def test_the_clip_builders_do_what_they_say():
    clip = clips.drift_clip(FRAMES, *PLANE, every=4, noise=0.0)
    assert clip.dtype == np.float32 and clip.shape == (FRAMES, *PLANE, 3)
    assert (clip[0] == clip[3]).all() and (clip[3, :, 1:] == clip[4, :, :-1]).all() and (clip[0, :, 11:] == clip[47, :, :-11]).all()
    noisy = clips.drift_clip(FRAMES, *PLANE)
    assert noisy.dtype == np.float32 and 0.005 < np.std(noisy - clip) < 0.015
    images, mask = fill_clip()
    y, x = clips.box_of(*PLANE)
    assert (mask.sum(axis=(1, 2)) == np.where(np.arange(FRAMES) < LEAVES, 80, 25)).all()
    assert mask[0, y:y + 8, x:x + 10].all() and mask[LEAVES, -5:, :5].all() and not mask[LEAVES, y:y + 8, x:x + 10].any()
    changed, mask = checked_clip()
    assert (mask.sum(axis=(1, 2)) == np.where((np.arange(FRAMES) >= ARRIVES) & (np.arange(FRAMES) < LEAVES), 80, 25)).all()
    diff = changed - images
    assert not diff[:CHANGE].any() and (diff[CHANGE:] != 0).any(axis=(0, 3)).sum() > 0
    where = (diff[CHANGE] != 0).any(axis=-1)
    assert (where & (mask[CHANGE] == 1)).any() and (where & (mask[CHANGE] == 0)).any()        # the box's left part and known pixels
    assert not where[:, x + 3:].any() and (np.abs(diff[CHANGE:][:, where] - 0.35) < 1e-6).all()
    assert 0.25 < clips.random_mask(SMOOTH_FRAMES, *PLANE).mean() < 0.35


def test_plain_fill_origins_are_tens_of_frames_old():
    images, mask = fill_clip()
    filled, remaining, source = fill_want(0)
    age = ages(mask, source)
    assert age.max() == LEAVES == 40                                   # frame 0 waits for the frame in which the box has left
    assert (age >= 32).sum() >= 100                                    # [120]
    assert not remaining.any() and (_bits(filled) != _bits(images)).any(axis=-1)[mask == 1].all()


def test_reach_at_the_largest_age_changes_nothing_and_one_below_it_does():
    images, mask = fill_clip()
    assert same_bits(fill_want(40), fill_want(0))
    at, below = fill_want(40), fill_want(39)
    lost = (below[1] == 1) & (at[1] == 0)
    assert lost.any() and not at[1].any()                              # [8 pixels, all of frame 0]
    assert ages(mask, below[2]).max() == 39


def test_a_short_reach_bounds_the_age_and_leaves_most_of_the_box():
    images, mask = fill_clip()
    filled, remaining, source = fill_want(7)
    assert ages(mask, source).max() == 7
    assert remaining.sum() > 1000                                      # [1820]
    assert ((remaining == 1) == ((mask == 1) & (source == tref.NONE))).all()


def test_one_mask_for_every_frame_still_borrows_from_far_away():
    images, mask = fill_clip(one_mask=True)
    filled, remaining, source = fill_want(0, True)
    assert mask.shape == PLANE and ages(mask, source).max() >= 32      # the canvas drifts out from under the box that stays


# ---- the checked fill --------------------------------------------------------------------------------------------------------------------
def test_the_scene_change_is_disputed_and_origins_are_old():
    images, mask = checked_clip()
    filled, remaining, source, witnesses = checked_want(0, 8)
    assert (source == cref.DISPUTED).sum() >= 100                      # [1890]
    assert set(np.unique(witnesses).tolist()) == {0, 1, 2} and (witnesses == 2).sum() >= 100      # [490]
    assert ages(mask, source).max() >= 16                              # [17]
    loose = checked_want(0, 255)                                       # nothing is far enough apart for agree = 255
    assert not (loose[2] == cref.DISPUTED).any() and not same_bits(loose, (filled, remaining, source, witnesses))
    short = checked_want(7, 8)
    assert ages(mask, short[2]).max() == 7 and (short[2] == cref.NONE).sum() > (source == cref.NONE).sum()
    assert set(np.unique(short[3]).tolist()) == {0, 1}                 # 34 frames of box: the two witnesses, 7 frames each, never meet


# ---- the smooth --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [3, 6])
def test_smooth_chains_run_their_full_eight_steps_both_ways(channels):
    images, mask = smooth_clip(SMOOTH_FRAMES, channels)
    out, support = smooth_want(SMOOTH_FRAMES, 8, 24, "picture", channels)
    assert (support == 16).sum() >= 100                                # [785 at 3 channels, 686 at 6]: the sum of weights is 4^8
    assert len(np.unique(support)) >= 8                                # [14, 12]
    full = support == 16
    assert (_bits(out) != _bits(images))[full][:, 4 if channels > 4 else 0:].any(axis=0).all()   # every channel of the last group moves


def test_the_shared_fields_give_the_whole_restatement():
    images, mask = smooth_clip(SMOOTH_FRAMES)
    whole = sref.temporal_smooth_ref(images, mask, 8, 24, "picture", LEVELS, SEARCH, SMOOTH)
    assert same_bits(whole, smooth_want(SMOOTH_FRAMES, 8, 24, "picture"))
    one = sref.temporal_smooth_ref(images, mask[0], 5, 255, "background", LEVELS, SEARCH, SMOOTH)
    assert same_bits(one, smooth_want(SMOOTH_FRAMES, 5, 255, "background", 3, True))


def test_smaller_radii_and_the_long_clip_reach_their_full_support_too():
    for radius in (5, 1):
        assert (smooth_want(SMOOTH_FRAMES, radius, 24, "background")[1] == 2 * radius).sum() >= 100
    assert (smooth_want(FRAMES, 8, 24, "picture")[1] == 16).sum() >= 1000
