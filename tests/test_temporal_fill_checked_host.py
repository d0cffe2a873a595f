"""The checked video temporal fill, the parts that need no device: what the rule promises, on the two restatements
(tests/temporal_fill_ref.py, tests/temporal_fill_checked_ref.py), as bits and counts; that the case of the device's stage test
reaches every branch of the rule; the C entry's argument checks (made before any HIP call), the wrappers' argument checks, the
node's protocol and the no-fallback errors.  Layouts, constants and names against the header are tests/test_cabi_mirror.py's, for
the whole C ABI."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi
from tests import temporal_fill_checked_ref as cref
from tests import temporal_fill_ref as tref
from tests.compare import _f32_bits as _bits
from tests.temporal_clips import (CLEAN_CLIPS, SECOND_OBJECT, check_clean, check_invariant, clean_clip, pair_case, pair_want, random_clip,
                                  second_object_clip, second_object_counts)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the case of the device's stage test ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plane", [(40, 70), (23, 33)], ids=lambda s: "x".join(map(str, s)))
def test_the_stage_case_reaches_every_branch_of_the_rule(plane):
    H, W = plane
    stats = {}
    _, (filled, source, remaining, witnesses) = pair_want(pair_case(H, W), True, 0, 8, stats)
    n, mu, flag = stats["n"], stats["mu"], stats["flag"]
    for name in ("both", "only_a", "only_b", "neither", "disputed"):
        assert stats[name].any(), name
    assert (flag == 0).any() and (flag == 1).any() and ((flag == 0) & (n >= cref.MIN_PIXELS)).any()
    assert ((n > 0) & (n < cref.MIN_PIXELS)).any() and (flag[n < cref.MIN_PIXELS] == 0).all()
    assert set(np.unique(witnesses)) == {0, 1, 2} and (source == cref.DISPUTED).any()
    # the unclamped bias of a tested block, from d itself
    raw = np.zeros_like(mu)
    for by, bx in np.argwhere(n >= cref.MIN_PIXELS):
        win = (slice(8 * by, 8 * by + 8), slice(8 * bx, 8 * bx + 8))
        raw[by, bx] = (2 * int(stats["d"][win][stats["both"][win]].sum()) + n[by, bx]) // (2 * n[by, bx])
    assert (mu == np.clip(raw, -32, 32)).all()
    if plane == (40, 70):
        assert (n == cref.MIN_PIXELS).any()                            # at the threshold, and below it above
        assert ((raw > 32) & (mu == 32)).any() and ((raw < -32) & (mu == -32)).any()
        assert W % 8 and flag[:, -1].any()                             # a disputed block cut by the plane's right edge
    else:
        assert H % 8 and W % 8 and (n[-1] >= cref.MIN_PIXELS).any()   # a tested block cut by the plane's lower edge
    # under agree = 255 nothing is disputed, under agree = 1 more is
    for agree, cmp in ((255, lambda a, b: a == 0), (1, lambda a, b: a >= b)):
        other = {}
        pair_want(pair_case(H, W), True, 0, agree, other)
        assert cmp(int(other["flag"].sum()), int(flag.sum())), agree


def test_block_statistics_one_block_at_a_time():
    both = np.zeros((9, 20), bool)
    d = np.zeros((9, 20), np.int64)
    both[:2, :8], d[:2, :8] = True, 40                                 # 16 pixels, all 40 above: mu clamps at 32, R = 16 * 8
    both[:2, 8:16], d[:2, 8:16] = True, -3                             # a small bias is forgiven entirely
    both[:2, 16:], d[:2, 16:] = True, 100                              # 8 pixels of a block cut by the edge: not enough
    both[8, :8], d[8, :8] = True, 100                                  # a row of the bottom blocks, 8 pixels
    n, mu, R, flag = cref.block_stats(both, d, 8)
    assert n.tolist() == [[16, 16, 8], [8, 0, 0]] and mu.tolist() == [[32, -3, 0], [0, 0, 0]]
    assert R.tolist() == [[128, 0, 0], [0, 0, 0]] and flag.tolist() == [[0, 0, 0], [0, 0, 0]]        # R > agree n is strict
    assert cref.block_stats(both, d, 7)[3].tolist() == [[1, 0, 0], [0, 0, 0]]
    d[0, :8] = -41                                                     # D = 8 * 40 - 8 * 41 = -8: floor((-16 + 16) / 32) = 0
    assert cref.block_stats(both, d, 8)[1][0, 0] == 0
    d[0, 0] = -42                                                      # D = -9: floor(-2 / 32) = -1, the mathematical floor
    assert cref.block_stats(both, d, 8)[1][0, 0] == -1
    assert cref.sample_luma(np.array([[np.nan, np.inf, -np.inf], [1, 1, 1], [0.5, 7, 7]], np.float32)).tolist() == [149, 255, 217]
    assert cref.sample_luma(np.array([[0.5, 7], [np.nan, 1]], np.float32)).tolist() == [128, 0]


# ---- the properties, on the restatements ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def second_object_results():
    _, clip, mask = second_object_clip()
    return tref.temporal_fill_ref(clip, mask), cref.temporal_fill_checked_ref(clip, mask)


def test_the_second_object_is_disputed_rather_than_pasted():
    counts = second_object_counts(*second_object_results())
    assert counts["plain_wrong"] >= 400                                # the clip tests something
    assert 4 * counts["wrong"] <= counts["plain_wrong"]                # at most a quarter as many wrong pixels
    assert 100 * counts["verified_wrong"] <= 15 * counts["verified"]   # at most 15 % of the verified ones
    assert counts["filled"] >= 1000                                    # and the fill still fills
    assert counts == SECOND_OBJECT


@pytest.mark.parametrize("scene", ["second object", "pan", "still", "random"])
def test_outside_a_dispute_the_checked_fill_is_the_plain_fill(scene):
    if scene == "second object":
        images, mask = second_object_clip()[1:]
        plain, checked = second_object_results()
    else:
        images, mask = random_clip() if scene == "random" else clean_clip(scene, False)
        levels = 3 if scene == "random" else 4
        plain, checked = tref.temporal_fill_ref(images, mask, levels), cref.temporal_fill_checked_ref(images, mask, levels)
    check_invariant(images, plain, checked, scene)
    if scene in ("second object", "random"):
        assert (checked[2] == cref.DISPUTED).any() and (checked[3] == 2).any() and (checked[3] == 1).any()


@pytest.mark.parametrize("name,noisy", CLEAN_CLIPS)
def test_clean_geometry_is_never_disputed_with_and_without_noise(name, noisy):
    clip, mask = clean_clip(name, noisy)
    plain, checked = tref.temporal_fill_ref(clip, mask), cref.temporal_fill_checked_ref(clip, mask)
    check_clean(plain, checked)


def test_one_and_two_frames_and_the_last_frame():
    rng = np.random.default_rng(7)
    video = rng.random((3, 16, 17, 3), dtype=np.float32)
    mask = (rng.random((3, 16, 17)) < 0.4).astype(np.float32)
    filled, remaining, source, witnesses = cref.temporal_fill_checked_ref(video[:1], mask[:1], 3)
    assert (_bits(filled) == _bits(video[:1])).all() and (remaining == mask[:1]).all() and not witnesses.any()
    for frames in (2, 3):
        plain = tref.temporal_fill_ref(video[:frames], mask[:frames], 3)
        checked = cref.temporal_fill_checked_ref(video[:frames], mask[:frames], 3)
        check_invariant(video[:frames], plain, checked, frames)
        last = frames - 1                                              # no backward step: one witness at the most, no dispute
        assert (checked[3][last] == ((mask[last] == 1) & (checked[2][last] >= 0))).all() and (checked[2][last] >= -1).all()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_entry_rejects_bad_arguments_without_a_device(hip_lib):
    C, E, U = ctypes, _cabi.LP_E_INVALID, _cabi.LP_E_UNSUPPORTED
    side = _cabi.LP_VMASK_MAX_SIDE
    a = [C.c_void_p(4096 * (i + 1)) for i in range(12)]               # never dereferenced: validation comes before any HIP call
    names = [f for f, t in _cabi.LpTfillCarryPairDesc._fields_ if t is C.c_void_p]
    good = dict(frames=5, height=40, width=70, channels=3, frame=2, donor=3, reach=0, agree=8, **dict(zip(names, a)))
    call = lambda **change: hip_lib.lp_tfill_carry_pair(C.byref(_cabi.LpTfillCarryPairDesc(**{**good, **change})), None)   # noqa: E731
    assert len(names) == 12 and names[-1] == "witnesses" and hip_lib.lp_tfill_carry_pair(None, None) == E
    for change in ({"frames": 1}, {"frames": 0}, {"height": 0}, {"height": side + 1}, {"width": 0}, {"width": side + 1},
                   {"channels": 0}, {"channels": _cabi.LP_DETAIL_MAX_CHANNELS + 1}, {"reach": -1}, {"reach": _cabi.LP_TFILL_MAX_REACH + 1},
                   {"agree": 0}, {"agree": -1}, {"agree": 256}, {"frame": -1, "donor": 0}, {"frame": 4, "donor": 5}, {"donor": 1},
                   {"donor": 2}, {"donor": 4}, {"frame": 5, "donor": 6}, {"org_src": None}, {"pos_src": None}):
        assert call(**change) == E, change
    for name in names:
        if name not in ("org_src", "pos_src"):                         # the donor's state: both null is "none"
            assert call(**{name: None}) == E, name
    for out in ("org_dst", "pos_dst", "filled", "source", "remaining", "witnesses"):    # an output that is an input or another output
        for other in names:
            if other != out:
                assert call(**{out: good[other]}) == E, (out, other)
    assert call(frames=65536) == U


def test_the_header_says_the_checked_fill_words():
    header = open(os.path.join(ROOT, "include", "lanpaint_hip.h")).read()
    for word in ("Checked temporal fill", "a dispute never alters", "mu = floor((2 D + n) / (2 n))", "R > agree * n", "source = -2",
                 "witnesses = 2 when n >= LP_PROP_MIN_PIXELS", "wherever source != -2", "Frame F - 1 has no backward step"):
        assert word in header, word


# ---- the wrappers and the node --------------------------------------------------------------------------------------------------------
def test_the_wrappers_refuse_cpu_tensors_and_bad_arguments():
    from lanpaint_amd import temporal_fill as tf, temporal_fill_checked as tc
    images, mask = torch.zeros(4, 16, 16, 3), torch.zeros(4, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tc.temporal_fill_checked(images, mask)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tc.temporal_fill_checked(images.numpy(), mask)
    planes = (torch.zeros(2, 2, 2, dtype=torch.int32), torch.zeros(16, 16, dtype=torch.uint8), torch.zeros(16, 16, dtype=torch.uint8), None,
              images, images.clone(), torch.zeros(4, 16, 16, dtype=torch.int32), mask.clone(), torch.zeros(4, 16, 16, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tc.carry_pair(*planes, 1)
    # the numbers are checked before the tensors are looked at
    for bad in (dict(levels=0), dict(levels=7), dict(search=0), dict(search=8), dict(smooth=-1), dict(smooth=65), dict(reach=-1),
                dict(reach=65536), dict(reach=1.0), dict(agree=0), dict(agree=256), dict(agree=8.0), dict(agree=True), dict(agree=None)):
        with pytest.raises(ValueError):
            tc.temporal_fill_checked(images, mask, **bad)
    for bad in (dict(reach=-1), dict(reach=65536), dict(agree=0), dict(agree=256)):
        with pytest.raises(ValueError):
            tc.carry_pair(*planes, 1, **bad)
    assert tc.DISPUTED == -2 and tc.MAX_AGREE == 255 and tf.WS_CAP_BYTES == 1 << 30
    assert "temporal_fill_checked" in tf.__doc__ and "a consistency check on it" not in tf.__doc__


def test_node_protocol_and_own_mappings():
    from lanpaint_amd import temporal_fill_checked_nodes as mod, temporal_fill_nodes
    node = mod.LanPaint_VideoTemporalFillChecked
    assert mod.NODE_CLASS_MAPPINGS == {"LanPaint_VideoTemporalFillChecked": node}
    assert list(mod.NODE_DISPLAY_NAME_MAPPINGS) == ["LanPaint_VideoTemporalFillChecked"]
    types = node.INPUT_TYPES()
    req, plain = types["required"], temporal_fill_nodes.LanPaint_VideoTemporalFill.INPUT_TYPES()["required"]
    assert list(types) == ["required"] and list(req) == list(plain) + ["agree"] and all(req[k] == plain[k] for k in plain)
    assert req["agree"][0] == "INT" and req["agree"][1] == {**req["agree"][1], "default": 8, "min": 1, "max": 255}
    for name in req:
        assert len(req[name][1]["tooltip"]) > 20, name
    for word in ("dispute", "disagree", "remaining", "mask fill", "encode", "Detailer", "verified", "colour-matched"):
        assert word in node.DESCRIPTION, word
    assert node.RETURN_TYPES == ("IMAGE", "MASK", "MASK", "MASK") and node.RETURN_NAMES == ("image", "remaining", "filled", "verified")
    assert node.FUNCTION == "fill" and callable(getattr(node, node.FUNCTION))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            node().fill(torch.zeros(3, 16, 16, 3), torch.zeros(3, 16, 16))
