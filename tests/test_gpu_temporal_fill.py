"""The video temporal fill on the MI355X (lanpaint_amd.temporal_fill, csrc/temporal_fill_kernel.hip) against the numpy restatement
tests/temporal_fill_ref.py.  Integer arithmetic decides everything but the final sample, and that is fp32 in a fixed order, so the
device must give the restatement's values whatever tile, batch or chunk a launch uses: every comparison covers every element and
has no tolerance.  Non-finite samples compare by being NaN on both sides, everything else by its bits.  Each stage is compared on
its own (fed with the restatement's inputs for that stage) and the whole call as well."""
import functools

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, propagate, temporal_fill as tf, temporal_fill_nodes
from tests import propagate_ref as ref
from tests import temporal_fill_ref as tref
from tests.test_gpu_propagate import (BIG, PLANES, _bits, _dev, _levels_of, _rng, _same, _soft, _threshold, _video, _wild_mask,
                                      _wild_video)
from tests.test_temporal_fill_host import check_fixed, check_pan, check_still, pan_clip, still_clip

pytestmark = pytest.mark.gpu
F, LEVELS = 5, 3
ALL_PLANES = PLANES + [BIG]
plane_ids = lambda s: "x".join(map(str, s))                          # noqa: E731


def _same_values(got, want, what):
    """fp32: NaN where the restatement has NaN, else the same bits."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    nan = np.isnan(want)
    bad = (np.isnan(got) != nan) | (~nan & (_bits(got) != _bits(want)))
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def _random_masks(frames, H, W, seed=0, share=0.3):
    return (_rng(frames, H, W, seed, 5).random((frames, H, W)) < share).astype(np.float32)


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
    frames, H, W = 18, 23, 33
    images, mask = _video(frames, H, W), _random_masks(frames, H, W)
    luma = propagate.luma_pyramids(_dev(images), LEVELS)
    known = tf.known_pyramids(_dev(mask), frames, LEVELS)
    steps = [(t, t - 1) for t in range(1, frames)] + [(t, t + 1) for t in range(frames - 2, -1, -1)]
    assert len(steps) == 34 and len(steps) % tf.MAX_JOBS == 2            # two launches per level, a remainder of 2
    got = tf.step_fields(luma, known, steps, H, W, LEVELS, 2, 8)
    assert got.dtype == torch.int32 and tuple(got.shape) == (34, *_cabi.prop_grid(H, W), 2)
    Y = ref.luma(images)
    pyr = [ref.pyramid(Y[f], LEVELS, ref.down_luma) for f in range(frames)]
    kpyr = tref.known_pyramids(tref.known_bits(mask, frames), LEVELS)
    host = got.cpu().numpy()
    for j, (t, s) in enumerate(steps):
        parent = None
        for lv in range(LEVELS - 1, -1, -1):
            vec, ok = propagate.match_level(luma[t], luma[s], known[t], H, W, LEVELS, lv, 2, 8, parent)
            parent = propagate.fill_median(vec, ok)
        assert torch.equal(got[j], parent), ("the single entries", j, t, s)
        _same(host[j], tref.step_field(pyr[t], pyr[s], kpyr[t], 2, 8), ("the restatement", j, t, s))


# ---- stages 3 and 4: one carry, fed with the restatement's inputs ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _carry_case(H, W, wild, channels=3):
    """A frame 2 of 5 with random known bits, a random field of up to 2.5 pixels, a random state of both neighbours with origins
    in every frame, and a random `source` under the mask from an earlier pass."""
    rng = _rng(H, W, int(wild), 6)
    images = (_wild_video if wild else _video)(F, H, W, channels)
    gh, gw = ref.grid_of(H, W)
    vec = rng.integers(-40, 41, (gh, gw, 2)).astype(np.int32)
    known = (rng.random((3, H, W)) < 0.5).astype(np.uint8)            # of the frames 1, 2, 3
    org = rng.integers(-1, F, (H, W)).astype(np.int32)
    pos = np.stack([rng.integers(-40, 16 * H + 40, (H, W)), rng.integers(-40, 16 * W + 40, (H, W))], axis=-1).astype(np.int32)
    source = np.where(known[1] != 0, 2, rng.choice([-1, 0, 1, 3, 4], (H, W))).astype(np.int32)
    return images, vec, known, org, pos, source


def _check_carry(H, W, wild, donor, state, reach, nearer, channels=3):
    t = 2
    images, vec, known, org, pos, source_t = _carry_case(H, W, wild, channels)
    known_t, known_s = known[1], known[donor - 1]
    want_org, want_pos = tref.carry(t, known_t, donor, known_s, vec, (org, pos) if state else None, reach)
    write = tref.choose(t, known_t, want_org, source_t, nearer)
    source = np.full((F, H, W), -7, np.int32)
    source[t] = source_t
    remaining = np.full((F, H, W), 0.25, np.float32)
    remaining[t] = (known_t == 0) & (source_t == -1)
    filled = images.copy()
    want_filled, want_source, want_remaining = filled.copy(), source.copy(), remaining.copy()
    want_filled[t][write] = tref.sample(images, want_org[write], want_pos[write][:, 0], want_pos[write][:, 1])
    want_source[t][write] = want_org[write]
    want_remaining[t][write] = 0
    d_filled, d_source, d_remaining = _dev(filled), _dev(source), _dev(remaining)
    got_org, got_pos = tf.carry(_dev(vec), _dev(known_t), _dev(known_s), (_dev(org), _dev(pos)) if state else None, _dev(images),
                                d_filled, d_source, d_remaining, t, donor, reach, nearer)
    what = ((H, W), wild, donor, state, reach, nearer, channels)
    under = known_t == 0                                               # the state planes matter under the mask only
    _same(got_org.cpu().numpy()[under], want_org[under], (what, "org"))
    _same(got_pos.cpu().numpy()[under], want_pos[under], (what, "pos"))
    _same_values(d_filled.cpu().numpy(), want_filled, (what, "filled"))
    _same(d_source.cpu().numpy(), want_source, (what, "source"))
    _same_values(d_remaining.cpu().numpy(), want_remaining, (what, "remaining"))
    return want_org, write


@pytest.mark.parametrize("plane", ALL_PLANES, ids=plane_ids)
def test_carry_equals_the_restatement(plane):
    H, W = plane
    for donor in (1, 3):                                               # the forward and the backward direction
        for nearer in (False, True):                                   # write always, write if nearer
            for state, reach in ((True, 0), (True, 1), (True, 2), (False, 0)):    # ages are 0, 1 and 2: reach at and one below
                _check_carry(H, W, False, donor, state, reach, nearer)
    _check_carry(H, W, True, 1, True, 0, False)
    _check_carry(H, W, True, 3, True, 2, True)


# One block high with several across, and the other way round: the grid is one block wide, so both blocks a pixel interpolates
# between are the same clamped one.  The plane list's own thin planes (1 x 1, 1 x 7, 7 x 1) are thinner than the case's vectors are
# long: there every masked pixel's vector leaves the plane and its value is never seen (counted on the restatement alone).
THIN_PLANES = [(7, 33), (33, 5)]


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


def _check_whole(got, want, what):
    for g, dtype in zip(got, (torch.float32, torch.float32, torch.int32)):
        assert g.is_cuda and g.dtype == dtype and g.is_contiguous()
    _same_values(got[0].cpu().numpy(), want[0], (what, "filled"))
    _same_values(got[1].cpu().numpy(), want[1], (what, "remaining"))
    _same(got[2].cpu().numpy(), want[2], (what, "source"))


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
