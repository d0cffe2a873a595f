"""The anchored video mask propagate on the MI355X (lanpaint_amd.propagate_anchored, lp_prop_anchor_match in
csrc/propagate_kernel.hip) against the numpy restatement tests/propagate_anchored_ref.py and against the existing matcher.  The rule
is integer arithmetic, so every comparison covers every element and has no tolerance.  The new launch is compared on its own, fed
with inputs made here, and the whole chain as well.  Without the feature this file fails at its imports."""
import functools

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, propagate, propagate_anchored, propagate_anchored_nodes, shots
from tests import propagate_anchored_ref as aref
from tests.anchor_clips import subpixel_clip
from tests.compare import _same_bits, _same_ints as _same
from tests.device import DEV, _dev
from tests.helpers import record_launches
from tests.inputs import ANCHORED_MASKS as MASKS, VISIBLE_PLANES as PLANES, _anchored_inputs as _inputs
from tests.motion_checks import _anchored_field as _device_field
from tests.propagate_scenes import assert_the_two_drift_iou_lines as assert_the_two_iou_lines, drift_case

pytestmark = pytest.mark.gpu
ANCHORS, SMOOTHS, POSITIONS, LUMAS = (1, 2, 7), (0, 8, 64), ("key", "smooth", "outside"), ("noisy", "flat")


# ---- inputs of the launch -------------------------------------------------------------------------------------------------------------
def _restatement_cases():
    """Every plane with every mask; the anchors, smooths, positions and lumas turn with the plane and the mask, so that every value
    of each meets every plane size class and every mask.  anchor 7 (225 candidates, four passes of the lanes) costs the restatement
    the most: on the two largest planes it keeps the disc and the random mask."""
    cases = []
    for i, plane in enumerate(PLANES):
        for j, mask in enumerate(MASKS):
            anchor = ANCHORS[(i + j) % 3]
            if anchor == 7 and plane[0] * plane[1] > 8000 and mask == "full":
                anchor = 2
            cases.append((plane, mask, anchor, SMOOTHS[(i + 2 * j) % 3], POSITIONS[(i // 3 + j) % 3], LUMAS[(i + j // 2) % 2]))
    cases.append(((70, 132), "disc", 7, 8, "smooth", "noisy"))          # several tiles, the vector path, four passes
    cases.append(((40, 70), "full", 7, 0, "outside", "flat"))
    return cases


def test_anchor_field_equals_the_restatement():
    cases = _restatement_cases()
    seen = {"valid": set()}
    for plane, mask, anchor, smooth, positions, lumas in cases:
        P, Yt, Yk, m = _inputs(plane, positions, lumas, mask)
        want_vec, want_valid = aref.anchor_field(P, Yt, Yk, m, anchor, smooth)
        vec, valid = _device_field(P, Yt, Yk, m, anchor, smooth)
        what = (plane, mask, anchor, smooth, positions, lumas)
        _same(valid, want_valid, ("valid", *what))
        _same(vec, want_vec, ("vec", *what))
        if mask == "empty":
            assert not want_valid.any() and not want_vec.any()
        seen["valid"].update((mask, bool(v)) for v in np.unique(want_valid))
        if want_vec.any():
            seen.setdefault("moved", set()).add((anchor, lumas))
        if (want_vec % 16 != 0).any():
            seen.setdefault("subpel", set()).add(anchor)
    for k, values in enumerate((ANCHORS, SMOOTHS, POSITIONS, LUMAS), start=2):
        assert {c[k] for c in cases} == set(values)
    assert {(c[0], c[1]) for c in cases} >= {(p, m) for p in PLANES for m in MASKS}
    assert {("full", True), ("disc", True), ("disc", False), ("random", True), ("random", False)} <= seen["valid"]
    assert {a for a, _ in seen["moved"]} == set(ANCHORS) and seen["subpel"] == set(ANCHORS)


def test_anchor_field_equals_the_existing_matcher_on_the_warped_key_luma():
    """K computed on the host and uploaded as a one-level pyramid: lp_prop_match with levels = 1 and search = anchor is the same
    rule (level 0 is the top level: no predictor, the sub-pixel step), so it gives the same vec and valid.  The device alone does
    the work here, so this runs every plane with every anchor, mask and kind of positions."""
    k = 0
    for plane in PLANES:
        H, W = plane
        stride = _cabi.prop_pyramid_ws_bytes(1, H, W, 1)

        def padded(a):
            buf = torch.zeros(stride, dtype=torch.uint8, device=DEV)
            buf[:H * W] = _dev(a).reshape(-1)
            return buf
        for positions in POSITIONS:
            for mask in MASKS:
                for anchor in ANCHORS:
                    smooth, lumas = SMOOTHS[k % 3], LUMAS[(k // 3) % 2]
                    k += 1
                    P, Yt, Yk, m = _inputs(plane, positions, lumas, mask)
                    K = aref.warped_key_luma(Yk, P)
                    want_vec, want_valid = propagate.match_level(padded(K), padded(Yt), padded(m), H, W, 1, 0, anchor, smooth)
                    vec, valid = propagate_anchored.anchor_field(_dev(P.astype(np.int32)), _dev(Yt), _dev(Yk), _dev(m), anchor, smooth)
                    what = (plane, positions, mask, anchor, smooth, lumas)
                    assert torch.equal(valid, want_valid), ("valid", *what)
                    assert torch.equal(vec, want_vec), ("vec", *what)


def test_anchor_field_on_unaligned_planes_takes_the_scalar_path_with_the_same_bits():
    """A width that is a multiple of 4 but planes that do not start on 16 bytes: views one element into a larger buffer."""
    P, Yt, Yk, m = _inputs((33, 64), "smooth", "noisy", "disc")
    want_vec, want_valid = aref.anchor_field(P, Yt, Yk, m, 2, 8)

    def shifted(a):
        buf = torch.empty(a.size + 1, dtype=torch.from_numpy(a[:0]).dtype, device=DEV)
        view = buf[1:].view(a.shape)
        view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        return view
    vec, valid = propagate_anchored.anchor_field(shifted(P.astype(np.int32)), shifted(Yt), _dev(Yk), shifted(m), 2, 8)
    _same(valid.cpu().numpy(), want_valid, "unaligned valid")
    _same(vec.cpu().numpy(), want_vec, "unaligned vec")


# ---- the whole chain ------------------------------------------------------------------------------------------------------------------
LEVELS = 3


@functools.lru_cache(maxsize=None)
def _clip(F, H, W, seed=0):
    images, truth = subpixel_clip(F, H, W, seed=seed)
    return images, truth


@functools.lru_cache(maxsize=None)
def _want(F, H, W, key):
    images, truth = _clip(F, H, W)
    return aref.propagate_anchored_ref(images, truth[key].astype(np.float32), key, LEVELS, 2, 8, 2)


@pytest.mark.parametrize("plane", [(23, 33), (40, 56)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("frames,key", [(1, 0), (2, 1), (7, 3), (33, 0)])
def test_the_chain_equals_the_restatement_bit_for_bit(plane, frames, key):
    H, W = plane
    if (frames, plane) == (33, (40, 56)):                              # the clip of the two IoU lines, at the default levels
        images, truth, plain, want = drift_case()
        got = propagate_anchored.propagate_masks_anchored(_dev(images), _dev(truth[0].astype(np.float32)))
        assert_the_two_iou_lines(truth, plain, got.cpu().numpy())
    else:
        images, truth = _clip(frames, H, W)
        want = _want(frames, H, W, key)
        got = propagate_anchored.propagate_masks_anchored(_dev(images), _dev(truth[key].astype(np.float32)), key, LEVELS, 2, 8, 2)
    assert got.is_cuda and got.dtype == torch.float32
    _same_bits(got.cpu().numpy(), want, ("mask", plane, frames, key))
    _same_bits(want[key], truth[key].astype(np.float32), "the key frame is the binarised mask")


def test_what_follows_from_the_rule_and_the_mask_forms():
    H, W = 23, 33
    images, truth = _clip(7, H, W)
    t, m = _dev(images), _dev(truth[3].astype(np.float32))
    want = _want(7, H, W, 3)
    per_frame = np.zeros((7, H, W), np.float32)
    per_frame[3] = truth[3]                                            # [F, H, W]: the key frame's mask is the one that is read
    for form in (_dev(per_frame), m[None]):
        _same_bits(propagate_anchored.propagate_masks_anchored(t, form, 3, LEVELS, 2, 8, 2).cpu().numpy(), want, "mask forms")
    assert not propagate_anchored.propagate_masks_anchored(t, torch.zeros_like(m), 3, LEVELS, 2, 8, 7).any()
    assert (propagate_anchored.propagate_masks_anchored(t, torch.ones_like(m), 3, LEVELS, 2, 8, 7) == 1).all()
    still = t[:1].repeat(3, 1, 1, 1)
    got = propagate_anchored.propagate_masks_anchored(still, m, 0, LEVELS, 2, 8, 7)
    _same_bits(got.cpu().numpy(), np.repeat(truth[3].astype(np.float32)[None], 3, axis=0), "equal frames")
    whole, truth1 = subpixel_clip(5, 40, 56, vy=0, vx=1, noise=0)      # a whole-pixel shift: e = 0, the plain chain's bits
    d, k = _dev(whole), _dev(truth1[0].astype(np.float32))
    assert torch.equal(propagate_anchored.propagate_masks_anchored(d, k, 0, 4, 2, 8, 2), propagate.propagate_masks(d, k, 0, 4, 2, 8))


STEP = ["lp_prop_match", "lp_prop_fill"] * LEVELS + ["lp_prop_advance", "lp_prop_anchor_match", "lp_prop_fill", "lp_prop_advance"]


def test_anchor_zero_is_propagate_masks_and_makes_no_new_launch(monkeypatch):
    H, W = 23, 33
    images, truth = _clip(7, H, W)
    t, m = _dev(images)[:4], _dev(truth[2].astype(np.float32))
    names = record_launches(monkeypatch, propagate_anchored, propagate)
    want = propagate.propagate_masks(t, m, 2, LEVELS, 2, 8)
    plain = list(names)
    assert "lp_prop_anchor_match" not in plain and plain.count("lp_prop_advance") == 3
    del names[:]
    got = propagate_anchored.propagate_masks_anchored(t, m, 2, LEVELS, 2, 8, 0)
    assert names == plain and torch.equal(got, want)                   # nothing but what propagate_masks launches itself
    del names[:]
    propagate_anchored.propagate_masks_anchored(t, m, 2, LEVELS, 2, 8, 2)
    assert [n for n in names if n not in ("lp_prop_luma", "lp_prop_key_mask")] == STEP * 3       # 2 levels + 4 launches a step
    assert [n for n in names if n in ("lp_prop_luma", "lp_prop_key_mask")] == [n for n in plain if n in ("lp_prop_luma", "lp_prop_key_mask")]


def test_one_frame_per_chunk_gives_the_bits_of_one_chunk_and_two_runs_the_same_bits(monkeypatch):
    """The chunks are propagate's (the new module reuses its chain_frames), so its cap is the one that is lowered; the key frame's
    luma has to outlive the chunk it came in."""
    H, W = 23, 33
    images, truth = _clip(7, H, W)
    t, m = _dev(images), _dev(truth[3].astype(np.float32))
    whole = propagate_anchored.propagate_masks_anchored(t, m, 3, LEVELS, 2, 8, 2)
    _same_bits(whole.cpu().numpy(), _want(7, H, W, 3), "one chunk")
    assert torch.equal(propagate_anchored.propagate_masks_anchored(t, m, 3, LEVELS, 2, 8, 2), whole)
    per_frame = _cabi.prop_pyramid_ws_bytes(1, H, W, LEVELS)
    for frames in (1, 2):
        monkeypatch.setattr(propagate_anchored.propagate, "WS_CAP_BYTES", frames * per_frame + 8)
        assert torch.equal(propagate_anchored.propagate_masks_anchored(t, m, 3, LEVELS, 2, 8, 2), whole), frames
    for bad in (dict(key_frame=7), dict(key_frame=-1), dict(anchor=8), dict(anchor=-1)):
        with pytest.raises(ValueError):
            propagate_anchored.propagate_masks_anchored(t, m, **bad)
    for bad_mask in (m[:-1], m[None].repeat(2, 1, 1), m[None, None]):
        with pytest.raises(ValueError):
            propagate_anchored.propagate_masks_anchored(t, bad_mask)


def test_two_clips_joined_at_a_cut_equal_the_two_separate_calls():
    H, W = 23, 33
    a, truth_a = _clip(4, H, W)
    b, truth_b = _clip(3, H, W, seed=1)
    joined, ranges = _dev(np.concatenate([a, b])), [(0, 4), (4, 7)]
    for key, (lo, hi), clip, mask in ((1, ranges[0], a, truth_a[1]), (6, ranges[1], b, truth_b[2])):
        m = _dev(mask.astype(np.float32))
        got = shots.propagate_masks_anchored_shots(joined, m, ranges, key, LEVELS, 2, 8, 2)
        want = propagate_anchored.propagate_masks_anchored(_dev(clip), m, key - lo, LEVELS, 2, 8, 2)
        assert torch.equal(got[lo:hi], want) and want.any(), key
        outside = torch.cat([got[:lo], got[hi:]])
        assert outside.numel() and (outside.view(torch.int32) == 0).all()          # exactly 0 in the other shot
    whole = shots.propagate_masks_anchored_shots(joined, _dev(truth_a[1].astype(np.float32)), [(0, 7)], 1, LEVELS, 2, 8, 2)
    assert torch.equal(whole, propagate_anchored.propagate_masks_anchored(joined, _dev(truth_a[1].astype(np.float32)), 1, LEVELS, 2, 8, 2))


def test_nodes_return_what_the_module_returns_on_the_inputs_device():
    H, W = 23, 33
    images, truth = _clip(7, H, W)
    mask = truth[3].astype(np.float32)
    node = propagate_anchored_nodes.LanPaint_VideoMaskPropagateAnchored()
    (out,) = node.propagate(torch.from_numpy(images), torch.from_numpy(mask), 3, LEVELS, 2, 8, 2)
    assert not out.is_cuda and out.dtype == torch.float32
    _same_bits(out.numpy(), _want(7, H, W, 3), "host in, host out")
    on_i, on_m = _dev(images), _dev(mask)
    (out,) = node.propagate(on_i, on_m, 3, LEVELS, 2, 8, 2)
    assert out.device == on_m.device and torch.equal(out, propagate_anchored.propagate_masks_anchored(on_i, on_m, 3, LEVELS, 2, 8, 2))
    (out,) = node.propagate(on_i, on_m)                                # the defaults: key 0, levels 4, search 2, smooth 8, anchor 2
    assert torch.equal(out, propagate_anchored.propagate_masks_anchored(on_i, on_m, 0, 4, 2, 8, 2))
    per_shot = propagate_anchored_nodes.LanPaint_VideoMaskPropagateAnchoredShots()
    (cut,) = per_shot.propagate(on_i, on_m, 3, LEVELS, 2, 8, 2, shots=[(0, 2), (2, 7)])
    assert torch.equal(cut[2:], propagate_anchored.propagate_masks_anchored(on_i[2:], on_m, 1, LEVELS, 2, 8, 2)) and not cut[:2].any()
    (same,) = per_shot.propagate(on_i, on_m, 3, LEVELS, 2, 8, 2)
    assert torch.equal(same, propagate_anchored.propagate_masks_anchored(on_i, on_m, 3, LEVELS, 2, 8, 2))
