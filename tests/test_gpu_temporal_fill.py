"""The video temporal fill on the MI355X (lanpaint_amd.temporal_fill, csrc/temporal_fill_kernel.hip) against the numpy restatement
tests/temporal_fill_ref.py.  Integer arithmetic decides everything but the final sample, and that is fp32 in a fixed order, so the
device must give the restatement's values whatever tile, batch or chunk a launch uses: every comparison covers every element and
has no tolerance.  Non-finite samples compare by being NaN on both sides, everything else by its bits.  Each stage is compared on
its own (fed with the restatement's inputs for that stage) and the whole call as well."""
import functools

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, temporal_fill as tf, temporal_fill_nodes
from tests import propagate_ref as ref
from tests import temporal_fill_ref as tref
from tests.compare import _f32_bits as _bits, _same_ints as _same, _same_values
from tests.device import _dev, _levels_of
from tests.inputs import (ALL_PLANES, FILL_FRAMES as F, FILL_LEVELS as LEVELS, THIN_PLANES, _carry_case, _random_masks, _soft, _threshold,
                          _video, _wild_mask, _wild_video, plane_ids)
from tests.motion_checks import _check_batched_fields, _check_carry, _check_fill_whole as _check_whole
from tests.temporal_clips import (check_fill_fixed as check_fixed, check_fill_pan as check_pan, check_fill_still as check_still,
                                  fill_pan_clip as pan_clip, fill_still_clip as still_clip)

pytestmark = pytest.mark.gpu


MASKS = {"empty": lambda n, H, W: np.zeros((n, H, W), np.float32), "full": lambda n, H, W: np.ones((n, H, W), np.float32),
         "threshold": lambda n, H, W: np.stack([_threshold(H, W, f) for f in range(n)]).astype(np.float32),
         "soft": lambda n, H, W: np.stack([_soft(H, W, f) for f in range(n)]),
         "wild": lambda n, H, W: np.stack([_wild_mask(H, W, f) for f in range(n)])}


# ---- stage 1: the known bits and their pyramids ----------------------------------------------------------------------------------------
def _check_known(mask, frames, levels, what, frame0=0):
    H, W = mask.shape[1:]
    known = tref.known_bits(mask, frames)
    source = torch.full((frames, H, W), 77, dtype=torch.int32, device=_dev(mask).device)
    remaining = torch.full((frames, H, W), 77.0, dtype=torch.float32, device=source.device)
    for planes in ((), (source, remaining, frame0)):
        pyr = tf.known_pyramids(_dev(mask), frames, levels, *planes)
        assert pyr.dtype == torch.uint8 and tuple(pyr.shape) == (frames, _cabi.prop_pyramid_ws_bytes(1, H, W, levels))
        got = _levels_of(pyr, H, W, levels)
        for f in range(frames):
            for lv, plane in enumerate(ref.pyramid(known[f], levels, ref.down_mask)):
                _same(got[lv][f], plane, (what, "known", f, lv))
    _same(source.cpu().numpy(), np.where(known != 0, frame0 + np.arange(frames)[:, None, None], -1), (what, "source"))
    _same_values(remaining.cpu().numpy(), (1 - known).astype(np.float32), (what, "remaining"))


@pytest.mark.parametrize("form", list(MASKS))
def test_known_pyramids_equal_the_restatement(form):
    for H, W in ALL_PLANES:
        _check_known(MASKS[form](F, H, W), F, LEVELS, (form, (H, W)))
    H, W = 23, 33
    _check_known(MASKS[form](1, H, W), 1, 6, (form, "one frame"))
    _check_known(MASKS[form](1, H, W), F, 1, (form, "one mask for every frame"))
    _check_known(MASKS[form](2, H, W), 2, LEVELS, (form, "a part of a clip"), frame0=65533)


# ---- stage 2: the fields -------------------------------------------------------------------------------------------------------------------
def test_batched_fields_equal_the_single_entries_and_the_restatement():
    _check_batched_fields()


# ---- stages 3 and 4: one carry, fed with the restatement's inputs ---------------------------------------------------------------------------
@pytest.mark.parametrize("plane", ALL_PLANES, ids=plane_ids)
def test_carry_equals_the_restatement(plane):
    H, W = plane
    for donor in (1, 3):                                               # the forward and the backward direction
        for nearer in (False, True):                                   # write always, write if nearer
            for state, reach in ((True, 0), (True, 1), (True, 2), (False, 0)):    # ages are 0, 1 and 2: reach at and one below
                _check_carry(H, W, False, donor, state, reach, nearer)
    _check_carry(H, W, True, 1, True, 0, False)
    _check_carry(H, W, True, 3, True, 2, True)


@pytest.mark.parametrize("plane", THIN_PLANES, ids=plane_ids)
def test_carry_on_a_grid_one_block_wide(plane):
    for donor in (1, 3):
        for state in (True, False):
            want_org, write = _check_carry(*plane, False, donor, state, 0, False)
            assert write.sum() >= 16                                   # vectors that stay inside the plane: origins found and sampled


def test_carry_case_covers_the_borders_the_reach_and_both_forms():
    H, W = 40, 70
    images, vec, known, org, pos, source_t = _carry_case(H, W, False)
    q = ref.key_positions(H, W) + ref.pixel_vectors(vec, H, W)
    under = known[1] == 0
    for side in (q[..., 0] < 0, q[..., 0] > 16 * (H - 1), q[..., 1] < 0, q[..., 1] > 16 * (W - 1)):
        assert (side & under).any()                                    # q leaves the plane on each of the four sides
    ages = {}
    for reach in (0, 1, 2):
        want_org, write = _check_carry(H, W, False, 1, True, reach, True)
        always = tref.choose(2, known[1], want_org, source_t, False)
        assert write.any() and (always & ~write).any()                 # some origins are nearer, some are not
        ages[reach] = np.abs(2 - want_org[under & (want_org >= 0)])
    assert ages[0].max() == 2 and ages[2].max() == 2 and ages[1].max() == 1 and len(ages[1]) < len(ages[2]) == len(ages[0])


# ---- the whole call ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(H, W, frames=F, channels=3, wild=False, levels=LEVELS, reach=0):
    images = (_wild_video if wild else _video)(frames, H, W, channels)
    mask = np.stack([_wild_mask(H, W, f) for f in range(frames)]) if wild else _random_masks(frames, H, W)
    return images, mask, tref.temporal_fill_ref(images, mask, levels, 2, 8, reach)


@pytest.mark.parametrize("plane", ALL_PLANES, ids=plane_ids)
def test_the_call_equals_the_restatement(plane):
    images, mask, want = _reference(*plane)
    _check_whole(tf.temporal_fill(_dev(images), _dev(mask), LEVELS, 2, 8), want, plane)
    if plane == (16, 17):
        assert ((want[2] >= 0) & (mask == 1)).any() and want[1].any()  # some pixels are borrowed and some remain


def test_the_call_on_the_wild_video_and_mask():
    images, mask, want = _reference(16, 17, wild=True)
    _check_whole(tf.temporal_fill(_dev(images), _dev(mask), LEVELS, 2, 8), want, "wild")
    images, mask, want = _reference(23, 33, wild=True, reach=1)
    _check_whole(tf.temporal_fill(_dev(images), _dev(mask), LEVELS, 2, 8, 1), want, "wild, reach 1")


@pytest.mark.parametrize("frames", [1, 2])
def test_one_and_two_frames(frames):
    images, mask, want = _reference(23, 33, frames=frames)
    _check_whole(tf.temporal_fill(_dev(images), _dev(mask), LEVELS, 2, 8), want, frames)
    if frames == 1:
        assert (_bits(want[0]) == _bits(images)).all()
    one = tref.temporal_fill_ref(images, mask[0], LEVELS, 2, 8)         # one mask for every frame, as [H, W] and [1, H, W]
    _check_whole(tf.temporal_fill(_dev(images), _dev(mask[0]), LEVELS, 2, 8), one, (frames, "[H, W]"))
    _check_whole(tf.temporal_fill(_dev(images), _dev(mask[:1]), LEVELS, 2, 8), one, (frames, "[1, H, W]"))


@pytest.mark.parametrize("channels", [1, 2, 3, 4])
def test_every_channel_count(channels):
    images, mask, want = _reference(23, 33, channels=channels)
    _check_whole(tf.temporal_fill(_dev(images), _dev(mask), LEVELS, 2, 8), want, channels)


def test_non_contiguous_and_fp16_input():
    H, W = 23, 33
    images, mask, want = _reference(H, W)
    wide = torch.zeros((F, H, 2 * W, 3), device=_dev(mask).device)
    wide[:, :, ::2] = _dev(images)
    strided = wide[:, :, ::2]
    assert not strided.is_contiguous()
    _check_whole(tf.temporal_fill(strided, _dev(mask).to(torch.float64), LEVELS, 2, 8), want, "non-contiguous")
    half = _dev(images).half()
    want = tref.temporal_fill_ref(half.float().cpu().numpy(), mask, LEVELS, 2, 8)
    _check_whole(tf.temporal_fill(half, _dev(mask).half(), LEVELS, 2, 8), want, "fp16")


def test_chunks_under_a_lowered_cap_and_a_second_call_give_the_same_bits(monkeypatch):
    H, W = 40, 70
    images, mask, want = _reference(H, W)
    t, m = _dev(images), _dev(mask)
    whole = tf.temporal_fill(t, m, LEVELS, 2, 8)
    _check_whole(whole, want, "one chunk")
    again = tf.temporal_fill(t, m, LEVELS, 2, 8)
    stride = _cabi.prop_pyramid_ws_bytes(1, H, W, LEVELS)
    gh, gw = _cabi.prop_grid(H, W)
    for steps in (1, 2, 3):                                            # 4 steps a direction: four chunks, two, and 3 + 1
        monkeypatch.setattr(tf, "WS_CAP_BYTES", 2 * stride + steps * (2 * stride + gh * gw * 8) + 8)
        chunked = tf.temporal_fill(t, m, LEVELS, 2, 8)
        for name, a, b, c in zip(("filled", "remaining", "source"), whole, again, chunked):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, "a second call")
            assert torch.equal(a.view(torch.int32), c.view(torch.int32)), (name, steps, "steps a chunk")


# ---- what follows from the rule, on the device ---------------------------------------------------------------------------------------------
def _run(clip, mask, **kw):
    return [o.cpu().numpy() for o in tf.temporal_fill(_dev(clip), _dev(mask), **kw)]


def test_pan_clip_is_filled_with_the_true_background_bit_for_bit():
    _, clip, mask = pan_clip()
    check_pan(*_run(clip, mask))


@pytest.mark.parametrize("reach", [1, 2, 8])
def test_reach_bounds_the_age_on_a_still_canvas(reach):
    _, clip, mask = still_clip(2)
    check_still(reach, *_run(clip, mask, reach=reach))


def test_a_fixed_subject_empty_and_full_masks_leave_the_images():
    _, clip, mask = still_clip(0)
    check_fixed(*_run(clip, mask))
    images = _video(F, 23, 33)
    for value in (0.0, 1.0):
        filled, remaining, source = _run(images, np.full((23, 33), value, np.float32), levels=LEVELS)
        assert (_bits(filled) == _bits(images)).all() and (remaining == value).all()
        assert (source == (np.arange(F)[:, None, None] if value == 0 else -1)).all()


def test_node_returns_what_the_module_returns_on_the_inputs_device():
    H, W = 23, 33
    images, mask, want = _reference(H, W)
    node = temporal_fill_nodes.LanPaint_VideoTemporalFill()
    image, remaining, filled = node.fill(torch.from_numpy(images), torch.from_numpy(mask), LEVELS, 2, 8, 0)
    assert not image.is_cuda and not remaining.is_cuda and not filled.is_cuda
    _same_values(image.numpy(), want[0], "host in, host out")
    _same_values(remaining.numpy(), want[1], "remaining")
    _same_values(filled.numpy(), mask - want[1], "filled = the mask's bits without remaining")
    on_i, on_m = _dev(images), _dev(mask)
    image, remaining, filled = node.fill(on_i, on_m, LEVELS, 2, 8, 0)
    direct = tf.temporal_fill(on_i, on_m, LEVELS, 2, 8, 0)
    assert image.device == on_i.device and torch.equal(remaining, direct[1]) and torch.equal(image.view(torch.int32), direct[0].view(torch.int32))
    image, _, _ = node.fill(torch.from_numpy(images), torch.from_numpy(mask))       # the defaults: levels 4, search 2, smooth 8, reach 0
    _same_values(image.numpy(), tref.temporal_fill_ref(images, mask)[0], "defaults")
