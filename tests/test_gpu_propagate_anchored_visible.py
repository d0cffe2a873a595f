"""The anchored occlusion-aware video mask propagate on the MI355X (lanpaint_amd.propagate_anchored_visible,
lp_prop_anchor_match_gated in csrc/propagate_kernel.hip) against the numpy restatement tests/propagate_anchored_visible_ref.py and
against the ungated launch.  The rule is integer arithmetic, so every comparison covers every element and has no tolerance.  The
new launch is compared on its own, fed with inputs made here, and the whole chain as well.  Without the feature this file fails at
its imports."""

import numpy as np
import pytest
import torch

from lanpaint_amd import (_cabi, propagate, propagate_anchored, propagate_anchored_visible, propagate_anchored_visible_nodes,
                          propagate_visible, shots)
from tests import propagate_anchored_visible_ref as avref
from tests.anchor_clips import subpixel_clip
from tests.compare import _same_bits, _same_ints as _same
from tests.device import DEV, _dev
from tests.helpers import record_launches
from tests.inputs import (ANCHORED_MASKS as MASKS, ANCHORED_VISIBLE_LEVELS as LEVELS, VISIBLE_PLANES as PLANES,
                          _anchored_visible_clip as _clip, _anchored_visible_inputs as _inputs, _anchored_visible_want as _want)
from tests.motion_checks import _anchored_visible_call as _call, _anchored_visible_field as _device_field
from tests.propagate_scenes import anchored_quality_case as quality_case, assert_the_anchored_quality_lines as assert_the_quality_lines

pytestmark = pytest.mark.gpu
ANCHORS, SMOOTHS, OCCLUSIONS, POSITIONS, LUMAS = (1, 2, 7), (0, 8, 64), (1, 16, 255), ("key", "smooth", "outside"), ("noisy", "dark")
# 1 x 1, 1 x 7, 8 x 8, 9 x 15: partial tiles and blocks; 33 x 64: the vector path; 70 x 132: several tiles
LAUNCH_PLANES = [(1, 1), (1, 7), (8, 8), (9, 15), (33, 64), (70, 132)]
assert set(LAUNCH_PLANES) <= set(PLANES)


# ---- inputs of the launch -------------------------------------------------------------------------------------------------------------
def _restatement_cases():
    """Every plane with every mask; the anchors, smooths, occlusions, positions and lumas turn with the plane and the mask, so
    that every value of each meets every mask.  anchor 7 (225 candidates, four passes of the lanes) costs the restatement the most:
    on the largest plane it keeps the disc."""
    cases = []
    for i, plane in enumerate(LAUNCH_PLANES):
        for j, mask in enumerate(MASKS):
            anchor = ANCHORS[(i + j) % 3]
            if anchor == 7 and plane == (70, 132) and mask != "disc":
                anchor = 2
            cases.append((plane, mask, anchor, SMOOTHS[(i + 2 * j) % 3], OCCLUSIONS[(2 * i + j) % 3], POSITIONS[(i // 3 + j) % 3],
                          LUMAS[(i + j // 2) % 2]))
    cases.append(((33, 64), "full", 7, 8, 16, "key", "noisy"))          # the match finds (1, -1): the gate follows the noise
    cases.append(((33, 64), "random", 2, 0, 16, "key", "noisy"))
    cases.append(((33, 64), "disc", 1, 64, 255, "smooth", "dark"))
    return cases


def test_gated_anchor_field_equals_the_restatement():
    cases = _restatement_cases()
    seen = set()
    for plane, mask, anchor, smooth, occlusion, positions, lumas in cases:
        P, Yt, Yk, m = _inputs(plane, positions, lumas, mask)
        want_vec, want_valid, want_gated = avref.gated_anchor_field(P, Yt, Yk, m, anchor, smooth, occlusion)
        vec, valid, gated = _device_field(P, Yt, Yk, m, anchor, smooth, occlusion)
        what = (plane, mask, anchor, smooth, occlusion, positions, lumas)
        _same(gated, want_gated, ("gated", *what))
        _same(valid, want_valid, ("valid", *what))
        _same(vec, want_vec, ("vec", *what))
        if mask == "empty":
            assert not want_valid.any() and not want_vec.any() and not want_gated.any()
        seen.update((mask, int(g)) for g in np.unique(want_gated))
        seen.update((mask, "valid", bool(v)) for v in np.unique(want_valid))
        if want_vec.any():
            seen.add(("moved", anchor))
    for k, values in enumerate((ANCHORS, SMOOTHS, OCCLUSIONS, POSITIONS, LUMAS), start=2):
        assert {c[k] for c in cases} == set(values)
    assert {(c[0], c[1]) for c in cases} >= {(p, m) for p in LAUNCH_PLANES for m in MASKS}
    assert {(mask, g) for mask in ("full", "disc", "random") for g in (0, 1)} <= seen
    assert {("full", "valid", True), ("disc", "valid", True), ("disc", "valid", False), ("random", "valid", True),
            ("random", "valid", False)} <= seen
    assert {("moved", a) for a in ANCHORS} <= seen


def test_gated_anchor_field_is_the_ungated_field_where_the_gate_is_open_and_zero_where_it_is_shut():
    """The characterisation, on the device alone, so every plane runs with every anchor, occlusion, mask and kind of positions:
    gated = 0: vec and valid are lp_prop_anchor_match's, bit for bit; gated = 1: valid = 0 and vec = 0, and the ungated launch
    found the block live."""
    k, seen = 0, set()
    for plane in PLANES:
        for positions in POSITIONS:
            for mask in MASKS:
                for anchor in ANCHORS:
                    for occlusion in OCCLUSIONS:
                        smooth, lumas = SMOOTHS[k % 3], LUMAS[(k // 3) % 2]
                        k += 1
                        P, Yt, Yk, m = _inputs(plane, positions, lumas, mask)
                        args = (_dev(P.astype(np.int32)), _dev(Yt), _dev(Yk), _dev(m), anchor, smooth)
                        want_vec, want_valid = propagate_anchored.anchor_field(*args)
                        vec, valid, gated = propagate_anchored_visible.gated_anchor_field(*args, occlusion)
                        what = (plane, positions, mask, anchor, smooth, occlusion, lumas)
                        shut = gated != 0
                        assert ((gated == 0) | (gated == 1)).all(), what
                        assert torch.equal(valid, torch.where(shut, 0, want_valid)), ("valid", *what)
                        assert torch.equal(vec, torch.where(shut[..., None], 0, want_vec)), ("vec", *what)
                        assert (want_valid[shut] == 1).all(), ("a gated block is live", *what)
                        seen.update((mask, int(g)) for g in torch.unique(gated).tolist())
    assert {(mask, g) for mask in ("full", "disc", "random") for g in (0, 1)} <= seen
    assert ("empty", 1) not in seen


def test_gated_anchor_field_on_unaligned_planes_takes_the_scalar_path_with_the_same_bits():
    """A width that is a multiple of 4 but planes that do not start on 16 bytes: views one element into a larger buffer."""
    P, Yt, Yk, m = _inputs((33, 64), "key", "noisy", "random")
    want_vec, want_valid, want_gated = avref.gated_anchor_field(P, Yt, Yk, m, 2, 0, 16)
    assert want_gated.any() and want_valid.any() and want_vec.any()

    def shifted(a):
        buf = torch.empty(a.size + 1, dtype=torch.from_numpy(a[:0]).dtype, device=DEV)
        view = buf[1:].view(a.shape)
        view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        return view
    vec, valid, gated = propagate_anchored_visible.gated_anchor_field(shifted(P.astype(np.int32)), shifted(Yt), _dev(Yk), shifted(m),
                                                                      2, 0, 16)
    _same(gated.cpu().numpy(), want_gated, "unaligned gated")
    _same(valid.cpu().numpy(), want_valid, "unaligned valid")
    _same(vec.cpu().numpy(), want_vec, "unaligned vec")


# ---- the whole chain ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plane", [(23, 33), (40, 56)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("frames,key", [(1, 0), (2, 1), (7, 3)])
def test_the_chain_equals_the_restatement_bit_for_bit(plane, frames, key):
    H, W = plane
    images, truth = _clip(frames, H, W, key)
    (want, want_hidden), trace = _want(frames, H, W, key)
    got, hidden = _call(_dev(images), _dev(truth[key].astype(np.float32)), key)
    assert got.is_cuda and hidden.is_cuda and got.dtype == hidden.dtype == torch.float32
    _same_bits(got.cpu().numpy(), want, ("mask", plane, frames, key))
    _same_bits(hidden.cpu().numpy(), want_hidden, ("hidden", plane, frames, key))
    _same_bits(want[key], truth[key].astype(np.float32), "the key frame is the binarised mask")
    assert not want_hidden[key].any()
    if frames > 1:                                                     # the clip does what it is for: the gate and the flags fire
        assert any(tr[2].any() for tr in trace.values()) and any(tr[6].any() for tr in trace.values())
        assert want_hidden.any() and any(tr[3].any() for tr in trace.values())


@pytest.mark.parametrize("name", ["A", "N"])
def test_the_quality_clips_at_the_defaults_equal_the_restatement_and_hold_the_quality_lines(name):
    """A: the occluded clip, the quality lines on the device's outputs of the three forms.  N: no occluder, the device's new form
    equals its anchored form and hides nothing."""
    images, truth, want, _, _ = quality_case(name)
    t, m = _dev(images), _dev(truth[0].astype(np.float32))
    got, hidden = propagate_anchored_visible.propagate_masks_anchored_visible(t, m)
    _same_bits(got.cpu().numpy(), want[0], ("mask", name))
    _same_bits(hidden.cpu().numpy(), want[1], ("hidden", name))
    anchored = propagate_anchored.propagate_masks_anchored(t, m)
    if name == "A":
        visible = propagate_visible.propagate_masks_visible(t, m)
        assert_the_quality_lines("A", truth, (got.cpu().numpy(), hidden.cpu().numpy()), anchored.cpu().numpy(),
                                 tuple(v.cpu().numpy() for v in visible))
    else:
        assert torch.equal(got, anchored) and not hidden.any()


def test_what_follows_from_the_rule_and_the_mask_forms():
    H, W = 23, 33
    images, truth = _clip(7, H, W, 3)
    t, m = _dev(images), _dev(truth[3].astype(np.float32))
    want, want_hidden = _want(7, H, W, 3)[0]
    per_frame = np.zeros((7, H, W), np.float32)
    per_frame[3] = truth[3]                                            # [F, H, W]: the key frame's mask is the one that is read
    for form in (_dev(per_frame), m[None]):
        got, hidden = _call(t, form, 3)
        _same_bits(got.cpu().numpy(), want, "mask forms")
        _same_bits(hidden.cpu().numpy(), want_hidden, "mask forms, hidden")
    got, hidden = _call(t, torch.zeros_like(m), 3, 7, 1)
    assert not got.any() and not hidden.any()                          # an empty mask gives 0 and 0
    still = t[3:4].repeat(3, 1, 1, 1)
    got, hidden = _call(still, m, 0, 7, 1)
    _same_bits(got.cpu().numpy(), np.repeat(truth[3].astype(np.float32)[None], 3, axis=0), "equal frames")
    assert not hidden.any()
    whole, truth1 = subpixel_clip(5, 40, 56, vy=0, vx=1, noise=0)      # a whole-pixel shift: the plain chain's bits, nothing hidden
    d, k = _dev(whole), _dev(truth1[0].astype(np.float32))
    got, hidden = propagate_anchored_visible.propagate_masks_anchored_visible(d, k)
    assert torch.equal(got, propagate.propagate_masks(d, k)) and not hidden.any()


STEP = ["lp_prop_match", "lp_prop_fill"] * LEVELS + ["lp_prop_advance", "lp_prop_anchor_match_gated", "lp_prop_fill", "lp_prop_advance",
                                                      "lp_prop_visible", "lp_prop_occlude"]
SETUP = ("lp_prop_luma", "lp_prop_key_mask")


def test_a_step_is_two_levels_plus_six_launches_and_the_off_forms_make_no_new_launch(monkeypatch):
    H, W = 23, 33
    images, truth = _clip(7, H, W, 3)
    t, m = _dev(images)[1:5], _dev(truth[3].astype(np.float32))
    names = record_launches(monkeypatch, propagate_anchored_visible, propagate_anchored, propagate_visible, propagate)
    new = ("lp_prop_anchor_match_gated",)
    for anchor, occlusion, base in ((0, 16, lambda: propagate_visible.propagate_masks_visible(t, m, 2, LEVELS, 2, 8, 16)),
                                    (2, 0, lambda: (propagate_anchored.propagate_masks_anchored(t, m, 2, LEVELS, 2, 8, 2), None)),
                                    (0, 0, lambda: (propagate.propagate_masks(t, m, 2, LEVELS, 2, 8), None))):
        del names[:]
        want, want_hidden = base()
        theirs = list(names)
        assert not set(new) & set(theirs) and theirs.count("lp_prop_advance") >= 3
        del names[:]
        got, hidden = _call(t, m, 2, anchor, occlusion)
        assert names == theirs, (anchor, occlusion)                    # nothing but what the other form launches itself
        assert torch.equal(got, want), (anchor, occlusion)
        assert torch.equal(hidden, want_hidden) if want_hidden is not None else (hidden.view(torch.int32) == 0).all()
    plain = [n for n in names if n in SETUP]
    del names[:]
    _call(t, m, 2)
    assert [n for n in names if n not in SETUP] == STEP * 3            # 2 levels + 6 launches a step
    assert len(STEP) == 2 * LEVELS + 6
    assert [n for n in names if n in SETUP] == plain


def test_one_frame_per_chunk_gives_the_bits_of_one_chunk_and_two_runs_the_same_bits(monkeypatch):
    """The chunks are propagate's (the new module reuses its chain_frames), so its cap is the one that is lowered; the key frame's
    luma has to outlive the chunk it came in."""
    H, W = 23, 33
    images, truth = _clip(7, H, W, 3)
    t, m = _dev(images), _dev(truth[3].astype(np.float32))
    whole = _call(t, m, 3)
    for got, want, what in zip(whole, _want(7, H, W, 3)[0], ("mask", "hidden")):
        _same_bits(got.cpu().numpy(), want, ("one chunk", what))
    again = _call(t, m, 3)
    assert torch.equal(again[0], whole[0]) and torch.equal(again[1], whole[1])
    per_frame = _cabi.prop_pyramid_ws_bytes(1, H, W, LEVELS)
    for frames in (1, 2):
        monkeypatch.setattr(propagate, "WS_CAP_BYTES", frames * per_frame + 8)
        names = record_launches(monkeypatch, propagate)
        got = _call(t, m, 3)
        assert names.count("lp_prop_luma") >= 7 // frames              # the chunks did get smaller
        assert torch.equal(got[0], whole[0]) and torch.equal(got[1], whole[1]), frames
    for bad in (dict(key_frame=7), dict(key_frame=-1), dict(anchor=8), dict(anchor=-1), dict(occlusion=256), dict(occlusion=-1)):
        with pytest.raises(ValueError):
            propagate_anchored_visible.propagate_masks_anchored_visible(t, m, **bad)
    for bad_mask in (m[:-1], m[None].repeat(2, 1, 1), m[None, None]):
        with pytest.raises(ValueError):
            propagate_anchored_visible.propagate_masks_anchored_visible(t, bad_mask)


def test_two_clips_joined_at_a_cut_equal_the_two_separate_calls():
    H, W = 23, 33
    a, truth_a = _clip(4, H, W, 1)
    b, truth_b = _clip(3, H, W, 2, seed=1)
    joined, ranges = _dev(np.concatenate([a, b])), [(0, 4), (4, 7)]
    for key, (lo, hi), clip, mask in ((1, ranges[0], a, truth_a[1]), (6, ranges[1], b, truth_b[2])):
        m = _dev(mask.astype(np.float32))
        got = shots.propagate_masks_anchored_visible_shots(joined, m, ranges, key, LEVELS, 2, 8, 2, 16)
        want = _call(_dev(clip), m, key - lo)
        assert isinstance(got, tuple) and len(got) == 2
        assert want[0].any() and want[1].any(), key
        for g, w in zip(got, want):
            assert torch.equal(g[lo:hi], w), key
            outside = torch.cat([g[:lo], g[hi:]])
            assert outside.numel() and (outside.view(torch.int32) == 0).all()      # exactly 0 in the other shot
    m = _dev(truth_a[1].astype(np.float32))
    whole = shots.propagate_masks_anchored_visible_shots(joined, m, [(0, 7)], 1, LEVELS, 2, 8, 2, 16)
    want = _call(joined, m, 1)
    assert torch.equal(whole[0], want[0]) and torch.equal(whole[1], want[1])


def test_nodes_return_what_the_module_returns_on_the_inputs_device():
    H, W = 23, 33
    images, truth = _clip(7, H, W, 3)
    mask = truth[3].astype(np.float32)
    want = _want(7, H, W, 3)[0]
    node = propagate_anchored_visible_nodes.LanPaint_VideoMaskPropagateAnchoredVisible()
    out = node.propagate(torch.from_numpy(images.copy()), torch.from_numpy(mask), 3, LEVELS, 2, 8, 2, 16)
    assert len(out) == 2
    for o, w, what in zip(out, want, ("mask", "hidden")):
        assert not o.is_cuda and o.dtype == torch.float32
        _same_bits(o.numpy(), w, ("host in, host out", what))
    on_i, on_m = _dev(images), _dev(mask)
    out = node.propagate(on_i, on_m, 3, LEVELS, 2, 8, 2, 16)
    direct = _call(on_i, on_m, 3)
    assert all(o.device == on_m.device and torch.equal(o, d) for o, d in zip(out, direct)) and len(out) == 2
    out = node.propagate(on_i, on_m)                                   # the defaults: key 0, levels 4, search 2, smooth 8, 2, 16
    direct = propagate_anchored_visible.propagate_masks_anchored_visible(on_i, on_m, 0, 4, 2, 8, 2, 16)
    assert all(torch.equal(o, d) for o, d in zip(out, direct))
    per_shot = propagate_anchored_visible_nodes.LanPaint_VideoMaskPropagateAnchoredVisibleShots()
    cut = per_shot.propagate(on_i, on_m, 3, LEVELS, 2, 8, 2, 16, shots=[(0, 2), (2, 7)])
    direct = _call(on_i[2:], on_m, 1)
    assert len(cut) == 2 and all(torch.equal(c[2:], d) and not c[:2].any() and c.shape[0] == 7 for c, d in zip(cut, direct))
    same = per_shot.propagate(on_i, on_m, 3, LEVELS, 2, 8, 2, 16)
    assert len(same) == 2 and all(torch.equal(s, d) for s, d in zip(same, _call(on_i, on_m, 3)))
