"""The checked video temporal fill on the MI355X (lanpaint_amd.temporal_fill_checked, lp_tfill_carry_pair in
csrc/temporal_fill_kernel.hip) against the numpy restatement tests/temporal_fill_checked_ref.py.  Integers decide everything but
the samples, and those are fp32 in a fixed order, so the device must give the restatement's values whatever tile or chunk a launch
uses: every comparison covers every element and has no tolerance (`_same`, `_same_values` of tests/test_gpu_temporal_fill.py).
The backward step is compared on its own, fed with the restatement's inputs, and the whole call as well."""
import functools

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, temporal_fill as tf, temporal_fill_checked as tc, temporal_fill_checked_nodes
from tests import temporal_fill_checked_ref as cref
from tests.compare import _same_values
from tests.device import _dev
from tests.inputs import (ALL_PLANES, FILL_FRAMES as F, FILL_LEVELS as LEVELS, THIN_PLANES, _random_masks, _video, _wild_mask,
                          _wild_video, plane_ids)
from tests.motion_checks import _check_checked_whole as _check_whole, _check_pair
from tests.temporal_clips import (CLEAN_CLIPS, SECOND_OBJECT, check_clean, check_invariant, clean_clip, pair_case, pair_want, random_clip,
                                  second_object_clip, second_object_counts)

pytestmark = pytest.mark.gpu


# ---- the backward step, fed with the restatement's inputs -----------------------------------------------------------------------------
@pytest.mark.parametrize("plane", ALL_PLANES, ids=plane_ids)
def test_carry_pair_equals_the_restatement(plane):
    H, W = plane
    for agree in (1, 8, 255):
        for state, reach in ((True, 0), (True, 1), (False, 0), (False, 1)):
            _check_pair(H, W, False, 3, state, reach, agree)
    for C in (1, 2, 4):
        _check_pair(H, W, False, C, True, 0, 8)
    _check_pair(H, W, True, 3, True, 0, 8)                             # NaN and infinities in the video
    _check_pair(H, W, True, 3, True, 1, 1)


@pytest.mark.parametrize("plane", THIN_PLANES, ids=plane_ids)
def test_carry_pair_on_a_grid_one_block_wide(plane):
    case = pair_case(*plane, False, 3)
    (want_org, _), _ = pair_want(case, True, 0, 8)
    assert ((case[2][0] == 0) & (want_org >= 0)).sum() >= 16           # masked pixels whose vector stays inside the plane
    for state in (True, False):
        _check_pair(*plane, False, 3, state, 0, 8)


def test_carry_pair_with_more_channels_than_one_gather_holds():
    _check_pair(23, 33, False, 6, True, 0, 8)
    _check_pair(23, 33, False, 9, True, 0, 255)


def test_carry_pair_refuses_the_last_frame():
    H, W = 16, 17
    images, vec, known, org, pos, source_t, filled_t = pair_case(H, W)
    planes = (_dev(vec), _dev(known[0]), _dev(known[1]), None, _dev(images), _dev(images.copy()), _dev(np.zeros((F, H, W), np.int32)),
              _dev(np.zeros((F, H, W), np.float32)), _dev(np.zeros((F, H, W), np.int32)))
    with pytest.raises(ValueError):
        tc.carry_pair(*planes, F - 1)


# ---- the whole call -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(H, W, frames=F, wild=False, one_mask=False, reach=0, agree=8):
    images = (_wild_video if wild else _video)(frames, H, W, 3)
    mask = np.stack([_wild_mask(H, W, f) for f in range(frames)]) if wild else _random_masks(frames, H, W)
    mask = mask[0] if one_mask else mask
    return images, mask, cref.temporal_fill_checked_ref(images, mask, LEVELS, 2, 8, reach, agree)


@pytest.mark.parametrize("plane", ALL_PLANES, ids=plane_ids)
def test_the_call_equals_the_restatement(plane):
    images, mask, want = _reference(*plane)
    _check_whole(tc.temporal_fill_checked(_dev(images), _dev(mask), LEVELS, 2, 8), want, plane)
    if plane == (40, 70):
        assert (want[2] == cref.DISPUTED).any() and {0, 1, 2} == set(np.unique(want[3]))


def test_the_call_on_the_wild_video_and_mask():
    images, mask, want = _reference(23, 33, wild=True, reach=1, agree=3)
    _check_whole(tc.temporal_fill_checked(_dev(images), _dev(mask), LEVELS, 2, 8, 1, 3), want, "wild, reach 1, agree 3")


@pytest.mark.parametrize("frames", [1, 2])
def test_one_and_two_frames_and_one_mask_for_every_frame(frames):
    images, mask, want = _reference(23, 33, frames=frames)
    _check_whole(tc.temporal_fill_checked(_dev(images), _dev(mask), LEVELS, 2, 8), want, frames)
    images, mask, want = _reference(23, 33, frames=frames, one_mask=True)
    _check_whole(tc.temporal_fill_checked(_dev(images), _dev(mask), LEVELS, 2, 8), want, (frames, "[H, W]"))
    _check_whole(tc.temporal_fill_checked(_dev(images), _dev(mask[None]), LEVELS, 2, 8), want, (frames, "[1, H, W]"))


def test_one_mask_for_every_frame_of_five():
    images, mask, want = _reference(23, 33, one_mask=True)
    _check_whole(tc.temporal_fill_checked(_dev(images), _dev(mask), LEVELS, 2, 8), want, "[H, W]")


def test_non_contiguous_and_fp16_input():
    H, W = 23, 33
    images, mask, want = _reference(H, W)
    wide = torch.zeros((F, H, 2 * W, 3), device=_dev(mask).device)
    wide[:, :, ::2] = _dev(images)
    strided = wide[:, :, ::2]
    assert not strided.is_contiguous()
    _check_whole(tc.temporal_fill_checked(strided, _dev(mask).to(torch.float64), LEVELS, 2, 8), want, "non-contiguous")
    half = _dev(images).half()
    want = cref.temporal_fill_checked_ref(half.float().cpu().numpy(), mask, LEVELS, 2, 8)
    _check_whole(tc.temporal_fill_checked(half, _dev(mask).half(), LEVELS, 2, 8), want, "fp16")


def test_chunks_under_a_lowered_cap_and_a_second_call_give_the_same_bits(monkeypatch):
    H, W = 40, 70
    images, mask, want = _reference(H, W)
    t, m = _dev(images), _dev(mask)
    whole = tc.temporal_fill_checked(t, m, LEVELS, 2, 8)
    _check_whole(whole, want, "one chunk")
    again = tc.temporal_fill_checked(t, m, LEVELS, 2, 8)
    stride = _cabi.prop_pyramid_ws_bytes(1, H, W, LEVELS)
    gh, gw = _cabi.prop_grid(H, W)
    for steps in (1, 2, 3):                                            # 4 steps a direction: four chunks, two, and 3 + 1
        monkeypatch.setattr(tf, "WS_CAP_BYTES", 2 * stride + steps * (2 * stride + gh * gw * 8) + 8)
        chunked = tc.temporal_fill_checked(t, m, LEVELS, 2, 8)
        for name, a, b, c in zip(("filled", "remaining", "source", "witnesses"), whole, again, chunked):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, "a second call")
            assert torch.equal(a.view(torch.int32), c.view(torch.int32)), (name, steps, "steps a chunk")


# ---- what follows from the rule, on the device ----------------------------------------------------------------------------------------
def _both(clip, mask, **kw):
    plain = [o.cpu().numpy() for o in tf.temporal_fill(_dev(clip), _dev(mask), **kw)]
    checked = [o.cpu().numpy() for o in tc.temporal_fill_checked(_dev(clip), _dev(mask), **kw)]
    return plain, checked


def test_the_second_object_is_disputed_rather_than_pasted():
    _, clip, mask = second_object_clip()
    plain, checked = _both(clip, mask)
    check_invariant(clip, plain, checked, "second object")
    counts = second_object_counts(plain, checked)
    assert counts["plain_wrong"] >= 400 and 4 * counts["wrong"] <= counts["plain_wrong"] and counts["filled"] >= 1000
    assert 100 * counts["verified_wrong"] <= 15 * counts["verified"]
    assert counts == SECOND_OBJECT


def test_outside_a_dispute_the_checked_fill_is_the_plain_fill_on_a_random_clip():
    images, mask = random_clip()
    plain, checked = _both(images, mask, levels=LEVELS)
    check_invariant(images, plain, checked, "random")
    assert (checked[2] == cref.DISPUTED).any()


@pytest.mark.parametrize("name,noisy", CLEAN_CLIPS[1:])                # pan, still and noisy; the noise-free pan clip is in the next test
def test_clean_geometry_is_never_disputed(name, noisy):
    plain, checked = _both(*clean_clip(name, noisy))
    check_clean(plain, checked)


def test_the_pan_clip_is_filled_with_the_true_background_and_verified():
    from tests.temporal_clips import check_fill_pan as check_pan
    plain, checked = _both(*clean_clip("pan", False))
    check_clean(plain, checked)
    check_pan(*checked[:3])


# ---- the node ---------------------------------------------------------------------------------------------------------------------------
def test_node_returns_what_the_module_returns_on_the_inputs_device():
    H, W = 23, 33
    images, mask, want = _reference(H, W)
    node = temporal_fill_checked_nodes.LanPaint_VideoTemporalFillChecked()
    image, remaining, filled, verified = node.fill(torch.from_numpy(images), torch.from_numpy(mask), LEVELS, 2, 8, 0, 8)
    assert not image.is_cuda and not remaining.is_cuda and not filled.is_cuda and not verified.is_cuda
    _same_values(image.numpy(), want[0], "host in, host out")
    _same_values(remaining.numpy(), want[1], "remaining")
    _same_values(filled.numpy(), mask - want[1], "filled = the mask's bits without remaining")
    _same_values(verified.numpy(), (want[3] == 2).astype(np.float32), "verified")
    on_i, on_m = _dev(images), _dev(mask)
    image, remaining, filled, verified = node.fill(on_i, on_m, LEVELS, 2, 8, 0, 8)
    direct = tc.temporal_fill_checked(on_i, on_m, LEVELS, 2, 8, 0, 8)
    assert image.device == on_i.device and torch.equal(remaining, direct[1]) and torch.equal(image.view(torch.int32), direct[0].view(torch.int32))
    assert torch.equal(verified, (direct[3] == 2).float())
    got = node.fill(torch.from_numpy(images), torch.from_numpy(mask))  # the defaults: levels 4, search 2, smooth 8, reach 0, agree 8
    default = cref.temporal_fill_checked_ref(images, mask)
    _same_values(got[0].numpy(), default[0], "defaults")
    _same_values(got[3].numpy(), (default[3] == 2).astype(np.float32), "defaults, verified")
