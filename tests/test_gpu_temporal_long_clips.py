"""The temporal fill, the checked fill and the temporal smooth on the MI355X where their own test modules do not go: clips of 20 and
48 frames (origins up to 40 frames old, `reach` at and one below that age, smooth chains of all 8 steps each way), more than
LP_PROP_MAX_JOBS = 32 steps in one whole call with chunks that straddle the job groups, 5 to 64 channels, the largest `levels`,
`search` and `smooth`, and a plane of 4 x 9 tiles.  Every comparison is with the numpy restatement, covers every element of every
output and has no tolerance (`_same`, `_same_values`): NaN matches NaN, everything else matches by its bits.  The long clips and
their restatement results are those of tests/test_temporal_long_clips_host.py, which asserts that they go where this file needs
them to."""
import functools

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, temporal_fill as tf, temporal_fill_checked as tc, temporal_smooth as ts
from lanpaint_amd._hostcall import chunks
from tests import temporal_fill_checked_ref as cref
from tests import temporal_fill_ref as tref
from tests import temporal_smooth_ref as sref
from tests.compare import _f32_bits as _bits
from tests.device import _dev
from tests.inputs import _carry_case, _random_masks, _video
from tests.motion_checks import (_check_carry, _check_checked_whole as _check_whole_checked, _check_fill_whole as _check_whole,
                                 _check_pair, _check_smooth)
from tests.temporal_clips import (LONG_FRAMES as FRAMES, LONG_LEVELS as LEVELS, LONG_PLANE as PLANE, LONG_SEARCH as SEARCH,
                                  LONG_SMOOTH as SMOOTH, LONG_SMOOTH_FRAMES as SMOOTH_FRAMES, long_checked_clip as checked_clip,
                                  long_checked_want as checked_want, long_fill_clip as fill_clip, long_fill_want as fill_want,
                                  long_smooth_clip as smooth_clip, long_smooth_want as smooth_want)

pytestmark = pytest.mark.gpu
PARAMS = (LEVELS, SEARCH, SMOOTH)
H, W = PLANE
MANY_CHANNELS = [5, 7, 8, 64]                                          # a second trip of the loops over four channels: 1, 3, 4 of it, and 16 trips


def _fill(images, mask, reach=0, params=PARAMS):
    return tf.temporal_fill(_dev(images), _dev(mask), *params, reach)


def _checked(images, mask, reach=0, agree=8, params=PARAMS):
    return tc.temporal_fill_checked(_dev(images), _dev(mask), *params, reach, agree)


def _smooth(images, mask, radius=8, tolerance=24, motion="background", params=PARAMS):
    return ts.temporal_smooth(_dev(images), _dev(mask), radius, tolerance, motion, *params)


# ---- long clips, the whole call ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reach", [0, 7, 39, 40])
def test_plain_fill_on_48_frames(reach):
    _check_whole(_fill(*fill_clip(), reach), fill_want(reach), ("fill", reach))


@pytest.mark.parametrize("agree", [8, 255])
@pytest.mark.parametrize("reach", [0, 7])
def test_checked_fill_on_48_frames_with_a_scene_change(reach, agree):
    _check_whole_checked(_checked(*checked_clip(), reach, agree), checked_want(reach, agree), ("checked", reach, agree))


@pytest.mark.parametrize("motion", sref.MOTIONS)
@pytest.mark.parametrize("tolerance", [24, 255])
@pytest.mark.parametrize("radius", [8, 5, 1])
@pytest.mark.parametrize("frames", [SMOOTH_FRAMES, FRAMES])
def test_smooth_on_20_and_48_frames(frames, radius, tolerance, motion):
    want = smooth_want(frames, radius, tolerance, motion)
    _check_smooth(_smooth(*smooth_clip(frames), radius, tolerance, motion), want, ("smooth", frames, radius, tolerance, motion))
    assert (want[1] == 2 * radius).any()


def test_one_mask_for_every_frame_of_a_long_clip():
    images, mask = fill_clip(one_mask=True)
    assert mask.shape == PLANE
    _check_whole(_fill(images, mask), fill_want(0, True), "fill, [H, W]")
    images, mask = checked_clip(one_mask=True)
    _check_whole_checked(_checked(images, mask), checked_want(0, 8, True), "checked, [H, W]")
    for frames, motion in ((SMOOTH_FRAMES, "background"), (FRAMES, "picture")):
        images, mask = smooth_clip(frames, one_mask=True)
        _check_smooth(_smooth(images, mask, 8, 24, motion), smooth_want(frames, 8, 24, motion, 3, True), ("smooth, [H, W]", frames))


# ---- more than 32 steps in a call, and chunks that straddle the groups of 32 jobs ----------------------------------------------------------
def _fill_cap(steps):
    """temporal_fill.WS_CAP_BYTES under which a chunk holds `steps` steps of the long clip, and the chunks that gives."""
    stride = _cabi.prop_pyramid_ws_bytes(1, H, W, LEVELS)
    gh, gw = _cabi.prop_grid(H, W)
    per_step = 2 * stride + gh * gw * 8
    cap = 2 * stride + steps * per_step + 8
    return cap, [n for _, n in chunks(FRAMES - 1, per_step, cap - 2 * stride)]


FILL_CHUNKS = {33: [33, 14], 5: [5] * 9 + [2], 1: [1] * 47}            # 33 = 32 + 1: two launches per level, then one of 14


def test_the_unchunked_long_clip_has_more_steps_than_one_launch_takes():
    assert FRAMES - 1 > tf.MAX_JOBS == 32 and _fill_cap(FRAMES - 1)[0] < tf.WS_CAP_BYTES       # 47 steps: groups of 32 and 15


@pytest.mark.parametrize("steps", list(FILL_CHUNKS))
def test_plain_fill_in_chunks_equals_the_restatement(monkeypatch, steps):
    cap, sizes = _fill_cap(steps)
    assert sizes == FILL_CHUNKS[steps]
    monkeypatch.setattr(tf, "WS_CAP_BYTES", cap)
    _check_whole(_fill(*fill_clip()), fill_want(0), ("fill", steps, "steps a chunk"))


@pytest.mark.parametrize("steps", list(FILL_CHUNKS))
def test_checked_fill_in_chunks_equals_the_restatement(monkeypatch, steps):
    cap, sizes = _fill_cap(steps)
    assert sizes == FILL_CHUNKS[steps]
    monkeypatch.setattr(tf, "WS_CAP_BYTES", cap)
    _check_whole_checked(_checked(*checked_clip()), checked_want(0, 8), ("checked", steps, "steps a chunk"))


SMOOTH_CHUNKS = {1: [1] * 48, 7: [7] * 6 + [6], 33: [33, 15]}           # 33 frames read 40 + 33 fields: three launches per level


@pytest.mark.parametrize("motion,planes", [("background", 2), ("picture", 3)])
@pytest.mark.parametrize("frames", list(SMOOTH_CHUNKS))
def test_smooth_in_chunks_equals_the_restatement(monkeypatch, frames, motion, planes):
    radius = 8
    stride = _cabi.prop_pyramid_ws_bytes(1, H, W, LEVELS)
    gh, gw = _cabi.prop_grid(H, W)
    per_frame = planes * stride + 2 * gh * gw * 8
    cap = (2 * radius + frames) * per_frame + 8
    assert [n for _, n in chunks(FRAMES, per_frame, cap - 2 * radius * per_frame)] == SMOOTH_CHUNKS[frames]
    fwd, bwd = ts.field_steps(0, 33, FRAMES, radius)
    assert len(fwd) + len(bwd) == 72 > 2 * tf.MAX_JOBS
    monkeypatch.setattr(ts, "WS_CAP_BYTES", cap)
    _check_smooth(_smooth(*smooth_clip(FRAMES), radius, 24, motion), smooth_want(FRAMES, radius, 24, motion), ("smooth", frames, motion))


# ---- more than four channels -------------------------------------------------------------------------------------------------------------
def _moved(got, images, where, first=4):
    """Every channel from `first` on differs from the images somewhere in `where`."""
    return (_bits(got) != _bits(images))[where][:, first:].any(axis=0).all()


@pytest.mark.parametrize("channels", MANY_CHANNELS)
def test_carry_with_more_channels_than_one_gather_holds(channels):
    for plane in ((23, 33), (40, 70)):
        for donor, state, reach, nearer in ((1, True, 0, False), (3, True, 2, True), (3, False, 0, True)):
            want_org, write = _check_carry(*plane, False, donor, state, reach, nearer, channels)
            images, vec, known, org, pos, _ = _carry_case(*plane, False, channels)
            _, want_pos = tref.carry(2, known[1], donor, known[donor - 1], vec, (org, pos) if state else None, reach)
            sampled = tref.sample(images, want_org[write], want_pos[write][:, 0], want_pos[write][:, 1])
            assert write.sum() >= 20 and (_bits(sampled) != _bits(images[2][write]))[:, 4:].any(axis=0).all()


def test_carry_pair_with_64_channels():
    _check_pair(23, 33, False, 64, True, 0, 8)
    _check_pair(40, 70, False, 64, False, 1, 255)


@functools.lru_cache(maxsize=None)
def _short(call, plane, frames, channels, params):
    """(images, mask, the restatement's result) of a short random moving clip under random masks."""
    images, mask = _video(frames, *plane, channels), _random_masks(frames, *plane)
    if call == "fill":
        return images, mask, tref.temporal_fill_ref(images, mask, *params)
    if call == "checked":
        return images, mask, cref.temporal_fill_checked_ref(images, mask, *params)
    return images, mask, sref.temporal_smooth_ref(images, mask, 2, 60, "background", *params)


def _check_short(call, plane, frames, channels, params):
    images, mask, want = _short(call, plane, frames, channels, params)
    what = (call, plane, frames, channels, params)
    if call == "fill":
        _check_whole(_fill(images, mask, params=params), want, what)
    elif call == "checked":
        _check_whole_checked(_checked(images, mask, params=params), want, what)
    else:
        _check_smooth(_smooth(images, mask, 2, 60, params=params), want, what)
    return images, mask, want


CALLS = ["fill", "checked", "smooth"]


@pytest.mark.parametrize("channels", MANY_CHANNELS)
@pytest.mark.parametrize("call", CALLS)
def test_the_whole_calls_with_more_than_four_channels(call, channels):
    images, mask, want = _check_short(call, PLANE, 5, channels, PARAMS)
    changed = (want[1] > 0) if call == "smooth" else (mask == 1) & (want[2] >= 0)
    assert changed.sum() >= 100 and _moved(want[0], images, changed)


@pytest.mark.parametrize("channels", [6, 64])
def test_smooth_chains_of_eight_steps_in_every_channel_group(channels):
    images, mask = smooth_clip(SMOOTH_FRAMES, channels)
    want = smooth_want(SMOOTH_FRAMES, 8, 24, "picture", channels)
    _check_smooth(_smooth(images, mask, 8, 24, "picture"), want, ("smooth", channels))
    assert (want[1] == 16).sum() >= 100 and _moved(want[0], images, want[1] == 16)


# ---- the full parameter range, and a wider plane -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("call", CALLS)
def test_the_largest_levels_search_and_smooth(call):
    assert (_cabi.LP_PROP_MAX_LEVELS, _cabi.LP_PROP_MAX_SEARCH, _cabi.LP_PROP_MAX_SMOOTH) == (6, 7, 64)
    images, mask, want = _check_short(call, (40, 70), 3, 3, (6, 7, 64))
    assert (_bits(want[0]) != _bits(images)).any()


@pytest.mark.parametrize("call", CALLS)
def test_a_plane_of_four_by_nine_tiles_with_a_last_row_of_one_pixel(call):
    plane = (97, 261)                                                  # 3 x 32 + 1 and 8 x 32 + 5
    images, mask, want = _check_short(call, plane, 3, 3, (6, 2, 8))
    last = (_bits(want[0]) != _bits(images)).any(axis=(0, 3))
    assert last[96].any() and last[:, 256:].any()                      # the last tile row and the last tile column write


# ---- inputs as callers give them, on the long clip ------------------------------------------------------------------------------------------
def _strided(images):
    wide = torch.zeros((images.shape[0], H, 2 * W, images.shape[3]), device=_dev(images[:1]).device)
    wide[:, :, ::2] = _dev(images)
    strided = wide[:, :, ::2]
    assert not strided.is_contiguous()
    return strided


@pytest.mark.parametrize("call", CALLS)
def test_non_contiguous_and_fp16_input_of_48_frames(call):
    if call == "fill":
        (images, mask), want, check = fill_clip(), fill_want(0), _check_whole
        run, ref = (lambda i, m: tf.temporal_fill(i, m, *PARAMS)), (lambda i, m: tref.temporal_fill_ref(i, m, *PARAMS))
    elif call == "checked":
        (images, mask), want, check = checked_clip(), checked_want(0, 8), _check_whole_checked
        run, ref = (lambda i, m: tc.temporal_fill_checked(i, m, *PARAMS)), (lambda i, m: cref.temporal_fill_checked_ref(i, m, *PARAMS))
    else:
        (images, mask), want, check = smooth_clip(FRAMES), smooth_want(FRAMES, 8, 24, "picture"), _check_smooth
        run = lambda i, m: ts.temporal_smooth(i, m, 8, 24, "picture", *PARAMS)                 # noqa: E731
        ref = lambda i, m: sref.temporal_smooth_ref(i, m, 8, 24, "picture", *PARAMS)           # noqa: E731
    check(run(_strided(images), _dev(mask).to(torch.float64)), want, (call, "non-contiguous"))
    half = _dev(images).half()
    assert (half.float().cpu().numpy() != images).any()
    check(run(half, _dev(mask).half()), ref(half.float().cpu().numpy(), mask), (call, "fp16"))     # the values after the conversion
