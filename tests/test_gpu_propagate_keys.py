"""The video mask propagate from several keyframes on the MI355X (lanpaint_amd.propagate_keys, csrc/propagate_kernel.hip): the
batched step entries against the single entries, lp_prop_merge and the whole call against the numpy restatement
tests/propagate_keys_ref.py.  The chains are integer arithmetic and the merge is fp64 in a fixed order, so every comparison covers
every element and has no tolerance.  A chain of the restatement is computed once, at its longest, and shared by the cases that
need its beginning."""
import functools

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, propagate, propagate_keys, propagate_keys_nodes, stabilize
from tests import propagate_keys_ref as kref
from tests import propagate_ref as ref
from tests.compare import _f32_bits as _bits, _same_bits
from tests.device import DEV, _dev, _equal
from tests.helpers import record_launches
from tests.inputs import KEYS_SPECIAL as SPECIAL, MASKS, _disc, _rng, _soft, _video
from tests.motion_checks import _check_batched_entries

pytestmark = pytest.mark.gpu
ONE = np.float32(1.0).view(np.uint32)
BIG = (70, 130)                                                       # several workgroups of every kernel


# ---- the batched entries against the single entries --------------------------------------------------------------------------------------
@pytest.mark.parametrize("plane", [(1, 1), (7, 9), (33, 70), BIG], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("jobs", [1, 2, 5, 32])
def test_batched_entries_equal_the_single_entries(plane, jobs):
    """Job i goes from frame i to frame i + 1 of one video under a mask of its own; odd jobs carry positions, even jobs start from
    the key's, in one launch."""
    _check_batched_entries(plane, jobs)


def test_the_wrappers_refuse_more_jobs_than_a_launch_holds_and_mixed_planes():
    vec, valid = torch.zeros(2, 2, 2, dtype=torch.int32, device=DEV), torch.zeros(2, 2, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        propagate_keys.fill_median_batch([(vec, valid)] * 33)
    with pytest.raises(ValueError):
        propagate_keys.fill_median_batch([])
    with pytest.raises(ValueError):
        propagate_keys.fill_median_batch([(vec, valid), (vec[:1].contiguous(), valid[:1].contiguous())])
    assert len(propagate_keys.fill_median_batch([(vec, valid)] * 32)) == 32


# ---- the merge ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("span", [2, 3, 7, 65535])
def test_merge_equals_the_restatement(span):
    pairs = np.array([(a, b) for a in SPECIAL for b in SPECIAL], dtype=np.int64)        # every pair: equal and opposite signs
    for H, W in ((1, 1), (7, 9), (33, 70), BIG):
        for frames in range(1, 6):
            for first in {1, max(1, (span - frames) // 2), span - frames}:
                if first < 1 or first + frames - 1 > span - 1:
                    continue
                rng = _rng(span, H, W, frames, first)
                q = rng.integers(-5000, 5001, (2, frames, H, W))
                q[q == 0] = 1
                pick = rng.random((frames, H, W)) < 0.6
                chosen = pairs[rng.integers(0, len(pairs), (frames, H, W))]
                q[0][pick], q[1][pick] = chosen[..., 0][pick], chosen[..., 1][pick]
                got = propagate_keys.merge_gap(_dev(q[0].astype(np.int32)), _dev(q[1].astype(np.int32)), span, first).cpu().numpy()
                want = np.stack([kref.merge(q[0][f], q[1][f], span, first + f) for f in range(frames)])
                _same_bits(got, want, ("merge", span, (H, W), frames, first))
    # every special pair at every weight of a short gap, and at both ends of the longest
    qa, qb = _dev(pairs[:, 0].astype(np.int32).reshape(1, 1, -1)), _dev(pairs[:, 1].astype(np.int32).reshape(1, 1, -1))
    for j in sorted({1, span // 2, span - 1} | set(range(1, min(span, 8)))):
        if 1 <= j <= span - 1:
            got = propagate_keys.merge_gap(qa, qb, span, j).cpu().numpy()
            _same_bits(got, kref.merge(pairs[:, 0], pairs[:, 1], span, j).reshape(1, 1, -1), ("pairs", span, j))
            same = pairs[:, 0] == pairs[:, 1]                          # equal distances: the bits of the two masks
            assert (_bits(got)[0, 0][same] == np.where(pairs[:, 0][same] > 0, ONE, 0)).all()


# ---- the whole call ----------------------------------------------------------------------------------------------------------------------
F7 = 7
KEY_SETS = [[0], [3], [6], [0, 6], [2, 4], [0, 3, 6], [1, 5], list(range(F7))]
LEVELS, SEARCH, SMOOTH = 3, 2, 8


def _painted(form, H, W, k):
    """The mask painted on frame k: a function of the frame, so that a chain is the same in every key set that holds its key."""
    if form == "shapes":                                              # a different shape per key
        return MASKS[("disc", "soft", "16 pixels", "wild", "threshold", "full", "disc")[k]](H, W, k)
    if form == "soft":
        return _soft(H, W, k)
    return MASKS[form](H, W, k)


@functools.lru_cache(maxsize=None)
def _clip(plane, half):
    images = _video(F7, *plane, 3, seed=5)
    if half:
        images = images.astype(np.float16).astype(np.float32)
    return images, kref.luma_pyramids(images, LEVELS)


@functools.lru_cache(maxsize=None)
def _longest_chain(plane, half, form, k, d):
    bits = ref.binarise(_painted(form, *plane, k))
    return kref.run_chain(_clip(plane, half)[1], bits, k, d, k if d < 0 else F7 - 1 - k, LEVELS, SEARCH, SMOOTH)


def _whole(plane, form, keys, half=False):
    """(the device's result, the restatement's) for one case; the [K, H, W] and the [F, H, W] mask forms must agree."""
    H, W = plane
    images = _clip(plane, half)[0]
    masks = np.stack([_painted(form, H, W, k) for k in keys])
    chain = lambda i, k, d, length: {t: m for t, m in _longest_chain(plane, half, form, k, d).items() if abs(t - k) <= length}    # noqa: E731
    want = kref.propagate_keys_ref(images, masks, keys, LEVELS, SEARCH, SMOOTH, chain=chain)
    t = _dev(images).half() if half else _dev(images)
    got = propagate_keys.propagate_keys(t, _dev(masks), keys, LEVELS, SEARCH, SMOOTH)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (F7, H, W)
    _same_bits(got.cpu().numpy(), want, (plane, form, keys, half))
    if len(keys) < F7:
        per_frame = np.full((F7, H, W), 0.75, np.float32)             # what is not on a key frame is not read
        per_frame[keys] = masks
        _equal(propagate_keys.propagate_keys(t, _dev(per_frame), keys, LEVELS, SEARCH, SMOOTH), got, ("[F, H, W]", plane, form, keys))
    return got, want


@pytest.mark.parametrize("plane", [(1, 1), (9, 7), (40, 70), BIG], ids=lambda s: "x".join(map(str, s)))
def test_the_whole_call_equals_the_restatement_for_every_key_set(plane):
    H, W = plane
    for keys in KEY_SETS:
        got, want = _whole(plane, "disc", keys)
        for i, k in enumerate(keys):
            _same_bits(want[k], ref.binarise(_painted("disc", H, W, k)).astype(np.float32), "a key frame is its binarised mask")
        images, masks = _dev(_clip(plane, False)[0]), [_dev(_painted("disc", H, W, k)) for k in keys]
        if len(keys) == 1:                                            # K = 1 is propagate_masks, and [H, W] is accepted
            single = propagate.propagate_masks(images, masks[0], keys[0], LEVELS, SEARCH, SMOOTH)
            _equal(got, single, ("K = 1", plane, keys))
            _equal(propagate_keys.propagate_keys(images, masks[0], keys, LEVELS, SEARCH, SMOOTH), single, ("[H, W]", plane, keys))
        else:                                                         # outside the keys: propagate_masks with that key alone
            first = propagate.propagate_masks(images, masks[0], keys[0], LEVELS, SEARCH, SMOOTH)
            last = propagate.propagate_masks(images, masks[-1], keys[-1], LEVELS, SEARCH, SMOOTH)
            _equal(got[:keys[0] + 1], first[:keys[0] + 1], ("in front of the first key", plane, keys))
            _equal(got[keys[-1]:], last[keys[-1]:], ("behind the last key", plane, keys))


@pytest.mark.parametrize("form", ["empty", "full", "shapes", "soft"])
def test_the_whole_call_for_every_mask_form(form):
    for plane in ((9, 7), (40, 70)):
        for keys in ([0, 6], [2, 4], [0, 3, 6], [1, 5]):
            got, want = _whole(plane, form, keys)
            if form == "empty":
                assert (_bits(want) == 0).all()
            if form == "full":
                assert (_bits(want) == ONE).all()


def test_half_precision_images_and_a_still_video():
    for plane in ((9, 7), (40, 70)):
        _whole(plane, "disc", [1, 5], half=True)
        _whole(plane, "shapes", [0, 3, 6], half=True)
    H, W = 40, 70
    still = _dev(np.repeat(_video(1, H, W), F7, axis=0))
    soft = _soft(H, W, 3)
    got = propagate_keys.propagate_keys(still, _dev(np.repeat(soft[None], 3, axis=0)), [0, 2, 6], LEVELS, SEARCH, SMOOTH)
    _same_bits(got.cpu().numpy(), np.repeat(ref.binarise(soft).astype(np.float32)[None], F7, axis=0), "a still video")


def test_more_chains_than_one_launch_holds(monkeypatch):
    """A key on every even frame of 36: 35 chains of one step, so every stage of the step takes two launches (32 + 3)."""
    F, H, W = 36, 24, 40
    keys = list(range(0, F, 2))
    assert len(propagate_keys.chain_plan(F, keys)) == 35
    images = _video(F, H, W, 3, seed=2)
    masks = np.stack([MASKS[("disc", "soft", "full")[k % 3]](H, W, k) for k in keys])
    names = record_launches(monkeypatch, propagate_keys)
    got = propagate_keys.propagate_keys(_dev(images), _dev(masks), keys, LEVELS, SEARCH, SMOOTH)
    batched = [n for n in names if n.endswith("_batch")]
    assert len(batched) == 2 * (2 * LEVELS + 1) and names.count("lp_prop_merge") == 17
    _same_bits(got.cpu().numpy(), kref.propagate_keys_ref(images, masks, keys, LEVELS, SEARCH, SMOOTH), "35 chains")


def test_the_active_chains_are_no_prefix_of_the_plan_and_more_than_one_launch_holds(monkeypatch):
    """Keys on 0, 2, ..., 64 and on 69 of 70 frames: 64 chains of one step, then the two chains of the gap 64 to 69 with four.  Step
    1 takes three launches per stage (32 + 32 + 2 jobs); steps 2 to 4 run plan rows 64 and 65 alone, in the field walk's scratch
    rows 0 and 1."""
    F, H, W = 70, 9, 15
    keys = list(range(0, 65, 2)) + [69]
    plan = propagate_keys.chain_plan(F, keys)
    assert len(plan) == 66 and [c[3] for c in plan] == [1] * 64 + [4, 4]
    images = _video(F, H, W, 3, seed=5)
    masks = np.stack([MASKS[("disc", "soft", "full")[k % 3]](H, W, k) for k in keys])
    names = record_launches(monkeypatch, propagate_keys)
    got = propagate_keys.propagate_keys(_dev(images), _dev(masks), keys, LEVELS, SEARCH, SMOOTH)
    batched = [n for n in names if n.endswith("_batch")]
    assert len(batched) == (3 + 3) * (2 * LEVELS + 1) and names.count("lp_prop_merge") == 33
    _same_bits(got.cpu().numpy(), kref.propagate_keys_ref(images, masks, keys, LEVELS, SEARCH, SMOOTH), "66 chains")


def test_the_chains_of_a_step_share_their_launches(monkeypatch):
    """F = 7 with keys on both ends at 3 levels: two chains of 5 steps run side by side, 5 x 7 batched launches and not 10 x 7."""
    H, W = 40, 70
    images, masks = _dev(_clip((H, W), False)[0]), _dev(np.stack([_disc(H, W), _disc(H, W)]))
    names = record_launches(monkeypatch, propagate_keys)
    propagate_keys.propagate_keys(images, masks, [0, 6], LEVELS, SEARCH, SMOOTH)
    batched = [n for n in names if n.endswith("_batch")]
    assert len(batched) == 5 * (2 * LEVELS + 1) == 35
    assert batched[:7] == ["lp_prop_match_batch", "lp_prop_fill_batch"] * LEVELS + ["lp_prop_advance_batch"]
    assert names.count("lp_prop_merge") == 1 and names.count("lp_prop_luma") == 1
    assert not [n for n in names if n in ("lp_prop_match", "lp_prop_fill", "lp_prop_advance")]


# ---- the rest ----------------------------------------------------------------------------------------------------------------------------
def test_two_calls_small_chunks_and_the_pyramid_cap(monkeypatch):
    H, W = 40, 70
    keys = [1, 5]
    images = _dev(_clip((H, W), False)[0])
    masks = _dev(np.stack([_painted("shapes", H, W, k) for k in keys]))
    whole = propagate_keys.propagate_keys(images, masks, keys, LEVELS, SEARCH, SMOOTH)
    _equal(propagate_keys.propagate_keys(images, masks, keys, LEVELS, SEARCH, SMOOTH), whole, "two calls")
    half = propagate_keys.propagate_keys(images.half(), masks, keys, LEVELS, SEARCH, SMOOTH)
    pyramids = _cabi.prop_pyramid_ws_bytes(F7, H, W, LEVELS)
    assert pyramids < H * W * 3 * 4 * 2                               # the cap below holds the pyramids and one frame's conversion
    monkeypatch.setattr(propagate_keys, "WS_CAP_BYTES", pyramids + 8)
    monkeypatch.setattr(stabilize, "WS_CAP_BYTES", 1)                 # the distances one frame at a time
    names = record_launches(monkeypatch, propagate_keys)
    _equal(propagate_keys.propagate_keys(images.half(), masks, keys, LEVELS, SEARCH, SMOOTH), half, "one frame per chunk")
    assert names.count("lp_prop_luma") == F7
    _equal(propagate_keys.propagate_keys(images, masks, keys, LEVELS, SEARCH, SMOOTH), whole, "fp32 needs no conversion")
    monkeypatch.setattr(propagate_keys, "WS_CAP_BYTES", pyramids - 1)
    with pytest.raises(ValueError, match=f"{pyramids} bytes.*{pyramids - 1}"):
        propagate_keys.propagate_keys(images, masks, keys, LEVELS, SEARCH, SMOOTH)
    monkeypatch.undo()
    for bad_masks in (masks[:1], masks[:, :-1], masks[None], masks[0]):
        with pytest.raises(ValueError):
            propagate_keys.propagate_keys(images, bad_masks, keys)
    for bad_keys in ([5, 1], [1, 1], [1, 7], []):
        with pytest.raises(ValueError):
            propagate_keys.propagate_keys(images, masks, bad_keys)


def test_node_returns_what_the_module_returns():
    H, W = 40, 70
    images = _clip((H, W), False)[0]
    masks = np.stack([_painted("shapes", H, W, k) for k in (0, 3, 6)])
    node = propagate_keys_nodes.LanPaint_VideoMaskPropagateKeys()
    want = propagate_keys.propagate_keys(_dev(images), _dev(masks), [0, 3, 6], LEVELS, SEARCH, SMOOTH)
    out, = node.propagate(torch.from_numpy(images), torch.from_numpy(masks), "0, 3 6", LEVELS, SEARCH, SMOOTH)
    assert not out.is_cuda and out.dtype == torch.float32
    _equal(out, want.cpu(), "host in, host out")
    out, = node.propagate(_dev(images), _dev(masks), "0,3,6", LEVELS, SEARCH, SMOOTH)
    assert out.is_cuda
    _equal(out, want, "device in, device out")
    out, = node.propagate(torch.from_numpy(images), torch.from_numpy(masks[:1]))      # the defaults: key 0, levels 4, search 2, smooth 8
    _equal(out, propagate.propagate_masks(_dev(images), _dev(masks[0])).cpu(), "defaults")
