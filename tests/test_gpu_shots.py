"""The video shot detect on the MI355X (lanpaint_amd.shots, csrc/shot_kernel.hip) against the numpy restatement
tests/shots_ref.py.  The rule is integers throughout, so the device must give the restatement's values whatever tile or chunk a
launch uses: every comparison covers every element and has no tolerance.  The shot-aware forms are compared with the plain
functions called on each shot, bit for bit, and the fill with the restatement's composition as well."""
import ctypes

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, shots, shots_nodes
from lanpaint_amd import propagate, stabilize, temporal_fill, temporal_fill_checked, temporal_smooth
from lanpaint_amd import temporal_fill_nodes
from tests import shot_clips as clips
from tests import shots_ref as sref
from tests.compare import _same_ints as _same, _same_values
from tests.device import _dev
from tests.inputs import _random_scores, _rng, _video, _wild_video, plane_ids
from tests.motion_checks import _check_scores
from tests.shot_clips import FILL_LEVELS, expected_shot, fill_case, foreign_sources, scores

pytestmark = pytest.mark.gpu
F = 5
PLANES = [(9, 15), (23, 33), (40, 70), (70, 130)]      # one block and a cut one; odd sizes; more than one tile; a 3 x 5 grid of tiles
SMALL = [(1, 1), (5, 6), (3, 40), (8, 8)]              # smaller than one block, or one block wide


# ---- shot_scores ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 3, 4])
@pytest.mark.parametrize("plane", PLANES, ids=plane_ids)
def test_scores_equal_the_restatement_at_every_level_and_search(plane, channels):
    images = _video(F, *plane, channels)
    for level in range(4):
        for search in (1, 2, 3):
            want = _check_scores(images, level, search, (plane, channels, level, search))
            assert level or (want[:, 0] > 0).all()


@pytest.mark.parametrize("plane", SMALL, ids=plane_ids)
def test_a_plane_smaller_than_one_block(plane):
    images = _video(F, *plane, 3)
    for level in (0, 1, 2):
        for search in (1, 3):
            _check_scores(images, level, search, (plane, level, search))


def test_a_wild_clip_with_nan_and_infinities():
    for plane in ((23, 33), (40, 70)):
        images = _wild_video(F, *plane, 3)
        assert np.isnan(images).any() and np.isinf(images).any()
        for level, search in ((0, 1), (2, 2), (1, 3)):
            _check_scores(images, level, search, ("wild", plane, level, search))


def test_one_frame_two_frames_and_other_dtypes():
    images = _video(F, 23, 33, 3)
    score, n = shots.shot_scores(_dev(images[:1]))
    assert tuple(score.shape) == (0, 2) and n == 6 * 9
    assert shots.shot_decide(score, n).tolist() == [0]
    _check_scores(images[:2], 2, 2, "two frames")
    half = shots.shot_scores(_dev(images).to(torch.float16), 1, 2)[0]              # converted, then the same rule
    _same(half.cpu().numpy(), sref.shot_scores(_dev(images).to(torch.float16).float().cpu().numpy(), 1, 2)[0], "fp16")


def test_the_histograms_of_a_chunk():
    images = _video(F, 40, 70, 3)
    Y = sref.planes(images, 1)
    pyr = propagate.luma_pyramids(_dev(images), 2)
    score = torch.empty((F - 1, 2), dtype=torch.int64, device=pyr.device)
    hist = shots.measure_planes(pyr[0, _cabi.prop_level_offset(40, 70, 1):], pyr.shape[1], F, 20, 35, 2, score)
    _same(hist.cpu().numpy(), np.stack([sref.histogram(y) for y in Y]), "hist")
    _same(score.cpu().numpy(), sref.scores_of_planes(Y, 2), "score")


# ---- shot_decide ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames", [2, 3, 255, 256, 257, 1025, 65535])
def test_decide_equals_the_restatement(frames):
    found = 0
    for n, seed in ((1000, 0), (1 << 28, 1)):                          # the largest plane: the products reach 2^50
        score = _random_scores(frames, n, seed)
        assert score[:, 0].max() <= 255 * n
        dev = _dev(score)
        for window in (1, 4, 16):
            for ratio in (100, 200):
                for threshold, hist in ((16, 30), (1, 0), (255, 100)):
                    want = sref.shot_decide(score, n, threshold, hist, ratio, window)
                    got = shots.shot_decide(dev, n, threshold, hist, ratio, window)
                    assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == (frames,)
                    _same(got.cpu().numpy(), want, (frames, n, window, ratio, threshold, hist))
                    found = max(found, int(want[-1]))
    if frames >= 255:
        assert found > frames // 8                                     # the scan has something to add up
        equal = (np.diff(score[:, 0]) == 0).sum()
        assert equal > frames // 8


def test_decide_on_runs_of_equal_scores():
    n = 100
    score = np.array([[10, 0], [5000, 200], [5000, 200], [10, 0], [5000, 200]], np.int64)
    for ratio, window, want in ((100, 4, [0, 0, 1, 2, 2, 3]), (101, 4, [0] * 6), (101, 1, [0, 0, 0, 0, 0, 1])):
        assert shots.shot_decide(_dev(score), n, 16, 30, ratio, window).tolist() == want
    flat = np.tile(np.array([[5000, 200]], np.int64), (300, 1))
    assert shots.shot_decide(_dev(flat), n, 16, 30, 100, 16).tolist() == list(range(301))
    assert shots.shot_decide(_dev(flat), n, 16, 30, 101, 16).tolist() == [0] * 301


# ---- detect_shots ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(clips.CLIPS))
def test_detect_on_the_host_tests_clips_whole_and_in_chunks_of_two_frames(name, monkeypatch):
    images, starts = clips.CLIPS[name]()
    want_score, n, _ = scores(name)
    want = sref.shot_decide(want_score, n, shots.THRESHOLD, shots.HIST)
    if name != "close_cuts":
        assert want.tolist() == expected_shot(len(images), starts).tolist()
    dev = _dev(images)
    shot, score = shots.detect_shots(dev)
    _same(score.cpu().numpy(), want_score, (name, "score"))
    _same(shot.cpu().numpy(), want, (name, "shot"))
    assert shots.shot_ranges(shot) == sref.shot_ranges(want)
    launches = []
    measure = shots.measure_planes
    monkeypatch.setattr(shots, "measure_planes", lambda *a: launches.append(a[2]) or measure(*a))
    monkeypatch.setattr(shots, "WS_CAP_BYTES", 1)
    shot2, score2 = shots.detect_shots(dev)
    assert launches == [2] * (len(images) - 1)                         # every chunk holds two frames
    assert torch.equal(score2, score) and torch.equal(shot2, shot)
    if name == "close_cuts":
        _same(shots.detect_shots(dev, window=1)[0].cpu().numpy(), expected_shot(len(images), starts), "window 1")


# ---- the shot-aware forms on the two-shot clip ------------------------------------------------------------------------------------------------
def _equal(got, want, what):
    got, want = (got,) if torch.is_tensor(got) else got, (want,) if torch.is_tensor(want) else want
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, i)
        if g.dtype == torch.float32:
            _same_values(g.cpu().numpy(), w.cpu().numpy(), (what, i))
        else:
            _same(g.cpu().numpy(), w.cpu().numpy(), (what, i))


def _halves(fn, ranges, tensors, *args, frame_output=None):
    parts = []
    for lo, hi in ranges:
        out = fn(*(t[lo:hi] for t in tensors), *args)
        out = [out] if torch.is_tensor(out) else list(out)
        if frame_output is not None:
            out[frame_output] = torch.where(out[frame_output] >= 0, out[frame_output] + lo, out[frame_output])
        parts.append(out)
    return tuple(torch.cat(c) for c in zip(*parts))


def _inside(source, ranges):
    for lo, hi in ranges:
        s = source[lo:hi]
        assert ((s < 0) | ((s >= lo) & (s < hi))).all(), (lo, hi)


def test_the_fills_stay_inside_their_shots():
    images, mask, ranges, whole, composed = fill_case()
    di, dm = _dev(images), _dev(mask)
    shot = shots.detect_shots(di)[0]
    assert shots.shot_ranges(shot) == ranges
    got = shots.temporal_fill_shots(di, dm, shot, FILL_LEVELS)                     # the shot tensor, read there
    _equal(got, _halves(temporal_fill.temporal_fill, ranges, (di, dm), FILL_LEVELS, frame_output=2), "fill")
    _same_values(got[0].cpu().numpy(), composed[0], "filled")                      # and the restatement's composition
    _same(got[1].cpu().numpy(), composed[1], "remaining")
    _same(got[2].cpu().numpy(), composed[2], "source")
    _inside(got[2], ranges)
    plain = temporal_fill.temporal_fill(di, dm, FILL_LEVELS)[2].cpu().numpy()
    assert foreign_sources(plain, mask, ranges) >= 1 and foreign_sources(got[2].cpu().numpy(), mask, ranges) == 0
    checked = shots.temporal_fill_checked_shots(di, dm, ranges, FILL_LEVELS)
    _equal(checked, _halves(temporal_fill_checked.temporal_fill_checked, ranges, (di, dm), FILL_LEVELS, frame_output=2), "checked")
    _inside(checked[2], ranges)
    assert (checked[2] == _cabi.LP_TFILL_DISPUTED).sum() == (_halves(temporal_fill_checked.temporal_fill_checked, ranges, (di, dm),
                                                                     FILL_LEVELS)[2] == _cabi.LP_TFILL_DISPUTED).sum()
    one = _dev(mask[2:3])                                                          # one mask for every frame goes in whole
    _equal(shots.temporal_fill_shots(di, one, ranges, FILL_LEVELS),
           _halves(lambda a: temporal_fill.temporal_fill(a, one, FILL_LEVELS), ranges, (di,), frame_output=2), "one mask")
    _equal(shots.temporal_fill_shots(di, dm, [(0, len(images))], FILL_LEVELS), temporal_fill.temporal_fill(di, dm, FILL_LEVELS), "one range")


def test_smooth_stabilize_and_propagate_stay_inside_their_shots():
    images, mask, ranges, _, _ = fill_case()
    di, dm = _dev(images), _dev(mask)
    got = shots.temporal_smooth_shots(di, dm, ranges, 2, 24, "background", FILL_LEVELS)
    _equal(got, _halves(temporal_smooth.temporal_smooth, ranges, (di, dm), 2, 24, "background", FILL_LEVELS), "smooth")
    assert (got[1] > 0).any()
    jitter = _dev((_rng(6, 7).random(mask.shape) < 0.4).astype(np.float32))
    _equal(shots.stabilize_masks_shots(jitter, ranges, 1, 2), _halves(stabilize.stabilize_masks, ranges, (jitter,), 1, 2), "stabilize")
    assert not torch.equal(shots.stabilize_masks_shots(jitter, ranges, 1, 2), stabilize.stabilize_masks(jitter, 1, 2))
    lo, hi = ranges[1]
    for key in (lo, hi - 1, 0):
        (a, b), = [r for r in ranges if r[0] <= key < r[1]]
        got = shots.propagate_masks_shots(di, dm[key], ranges, key, FILL_LEVELS)
        want = propagate.propagate_masks(di[a:b], dm[key], key - a, FILL_LEVELS)
        _equal(got[a:b], want, ("propagate", key))
        outside = torch.cat([got[:a], got[b:]])
        assert outside.numel() and (outside.view(torch.int32) == 0).all()          # exactly 0, not -0
        _equal(shots.propagate_masks_shots(di, dm, ranges, key, FILL_LEVELS), got, ("a mask per frame", key))
    key = lo - 1                                                                   # the box lies under the key's mask
    assert shots.propagate_masks_shots(di, dm, ranges, key, FILL_LEVELS)[:lo].any()
    assert propagate.propagate_masks(di, dm, key, FILL_LEVELS)[lo:].any()          # the plain call runs on into the next scene


# ---- the nodes end to end on host tensors -----------------------------------------------------------------------------------------------------
def test_nodes_end_to_end_on_host_tensors():
    images, mask, ranges, _, composed = fill_case()
    hi_, hm = torch.from_numpy(images), torch.from_numpy(mask)
    found, count, summary = shots_nodes.LanPaint_VideoShots().detect(hi_)
    assert found == ranges and count == 2 and summary == "0-2, 3-5"
    assert shots_nodes.LanPaint_VideoShots().detect(hi_, window=1, level=0, search=1)[1] == 2
    node = shots_nodes.LanPaint_VideoTemporalFillShots()
    got = node.fill(hi_, hm, levels=FILL_LEVELS, shots=found)
    parent = temporal_fill_nodes.LanPaint_VideoTemporalFill()
    want = _halves(lambda a, b: parent.fill(a, b, levels=FILL_LEVELS), ranges, (hi_, hm))
    assert all(not t.is_cuda for t in got)
    _equal(got, want, "fill node")
    _same_values(got[0].numpy(), composed[0], "fill node against the restatement")
    _equal(node.fill(hi_, hm, levels=FILL_LEVELS), parent.fill(hi_, hm, levels=FILL_LEVELS), "without shots")
    sub, sub_mask = shots_nodes.LanPaint_VideoShotSelect().select(hi_, found, 1, hm)
    assert torch.equal(sub, hi_[3:]) and torch.equal(sub_mask, hm[3:])
    for cls, args in ((shots_nodes.LanPaint_VideoTemporalFillCheckedShots, dict(levels=FILL_LEVELS)),
                      (shots_nodes.LanPaint_VideoTemporalSmoothShots, dict(levels=FILL_LEVELS))):
        base = cls.__mro__[2]()
        fn = cls.FUNCTION
        _equal(getattr(cls(), fn)(hi_, hm, shots=found, **args), _halves(lambda a, b: getattr(base, fn)(a, b, **args), ranges, (hi_, hm)), fn)
    stab = shots_nodes.LanPaint_VideoMaskStabilizeShots().stabilize(hm, shots=found)
    _equal(stab, _halves(lambda a: stabilize.stabilize_masks(_dev(a.numpy())).cpu(), ranges, (hm,)), "stabilize node")
    out, = shots_nodes.LanPaint_VideoMaskPropagateShots().propagate(hi_, hm, key_frame=2, levels=FILL_LEVELS, shots=found)
    assert out.shape == hm.shape and not out[3:].any() and out[:3].any() and not out.is_cuda
    _equal(out[:3], propagate.propagate_masks(_dev(images[:3]), _dev(mask[2]), 2, FILL_LEVELS).cpu(), "propagate node")


# ---- the entries' refusals, with live pointers ------------------------------------------------------------------------------------------------
def test_bad_descriptors_are_refused_and_nothing_is_written(hip_lib):
    E, U = _cabi.LP_E_INVALID, _cabi.LP_E_UNSUPPORTED
    plane = torch.zeros((3, 40 * 70), dtype=torch.uint8, device=_dev(np.zeros(1)).device)
    hist = torch.full((3, 64), 7, dtype=torch.int32, device=plane.device)
    score = torch.full((2, 2), 7, dtype=torch.int64, device=plane.device)
    shot = torch.full((3,), 7, dtype=torch.int32, device=plane.device)
    good = dict(frames=3, height=40, width=70, search=2, plane=plane.data_ptr(), stride=40 * 70, hist=hist.data_ptr(), score=score.data_ptr())
    for change, code in (({"frames": 0}, E), ({"height": 0}, E), ({"width": _cabi.LP_VMASK_MAX_SIDE + 1}, E), ({"search": 4}, E),
                         ({"search": 0}, E), ({"stride": 40 * 70 - 1}, E), ({"plane": None}, E), ({"hist": None}, E), ({"score": None}, E),
                         ({"score": hist.data_ptr()}, E), ({"hist": plane.data_ptr()}, E), ({"frames": 65536}, U)):
        assert hip_lib.lp_shot_measure(ctypes.byref(_cabi.LpShotMeasureDesc(**{**good, **change})), None) == code, change
    good = dict(frames=3, threshold=16, hist=30, ratio=200, window=4, n_pixels=2800, score=score.data_ptr(), shot=shot.data_ptr())
    for change, code in (({"frames": 0}, E), ({"threshold": 0}, E), ({"threshold": 256}, E), ({"hist": 101}, E), ({"ratio": 99}, E),
                         ({"ratio": 10001}, E), ({"window": 0}, E), ({"window": 17}, E), ({"n_pixels": 0}, E), ({"score": None}, E),
                         ({"shot": None}, E), ({"shot": score.data_ptr()}, E), ({"frames": 65536}, U)):
        assert hip_lib.lp_shot_decide(ctypes.byref(_cabi.LpShotDecideDesc(**{**good, **change})), None) == code, change
    torch.cuda.synchronize()
    assert (hist == 7).all() and (score == 7).all() and (shot == 7).all()
    with pytest.raises(ValueError):
        shots.shot_decide(score.to(torch.int32), 100)
    with pytest.raises(ValueError):
        shots.shot_decide(score.t(), 100)
