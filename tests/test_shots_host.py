"""The video shot detect, the parts that need no device: the properties the rule promises, on the restatement (tests/shots_ref.py)
and the clips of tests/shot_clips.py; the factor-2 margins of the default `threshold` and `hist`; `per_shot` with a stand-in
function on CPU tensors; the condition the shot-aware fill rests on, shown with the temporal fill's restatement alone; the C
entries' argument checks (made before any HIP call), the wrappers' argument checks and the nodes' protocol.  Layouts, constants
and names against the header are tests/test_cabi_mirror.py's, for the whole C ABI.

The margins.  The defaults are threshold 16 and hist 30, at the default level 2 and search 2.  On every clip here a pair that is
a cut has A / N >= 32 and a bin-change share >= 60 %.  A quiet pair -- a pan under noise -- has A / N <= 8 and a share <= 15 %.
The pairs of the fast large box are rejected by the histogram condition, which is what the rule has it for: their share is
<= 15 % (their residual, 10 .. 16 grey levels, has no such margin and is not asked for one).  The two pairs around a flash frame
pass both absolute conditions and are rejected by `ratio` alone: neither residual is twice the other.  Measured (level 2,
search 2): quiet pairs A / N 3.5 .. 4.0 and share 4 .. 11 %, box pairs 9.6 .. 15.8 and 6 .. 9 %, cuts 40.1 .. 88.3 and
85 .. 100 %, flash pairs 124 and 100 %."""
import ctypes
import os

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, shots, shots_nodes
from tests import shot_clips as clips
from tests import shots_ref as sref
from tests.shot_clips import expected_shot, fill_case, foreign_sources, scores

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, HI = shots.THRESHOLD, shots.HIST


# ---- the rule on the clips --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one_shot", "two_shots", "three_shots", "flash", "fast_box"])
def test_the_defaults_find_exactly_the_cuts(name):
    score, n, starts = scores(name)
    cut = sref.cuts(score, n, T, HI)
    assert np.flatnonzero(cut).tolist() == [k - 1 for k in starts], name
    shot = sref.shot_decide(score, n, T, HI)
    assert shot.dtype == np.int32 and shot.tolist() == expected_shot(len(score) + 1, starts).tolist()
    assert sref.shot_ranges(shot) == list(zip((0, *starts), (*starts, len(score) + 1)))


def test_a_flash_passes_the_absolute_conditions_and_falls_to_the_ratio():
    score, n, _ = scores("flash")
    at = clips.FLASH_AT
    for t in (at - 1, at):
        assert score[t, 0] >= 2 * T * n and 100 * score[t, 1] >= 2 * HI * 2 * n
    assert sref.cuts(score, n, T, HI, ratio=200).sum() == 0
    assert sref.cuts(score, n, T, HI, ratio=100).sum() == 1            # the larger of the two only


def test_a_fast_large_box_falls_to_the_histogram():
    score, n, _ = scores("fast_box")
    assert (score[:, 0] > 2 * score[:, 0].min()).sum() == 0 and score[:, 0].max() > 15 * n     # high residuals, none stands out
    assert sref.cuts(score, n, 1, HI, ratio=100, window=1).sum() == 0  # with the residual conditions as weak as they go
    assert sref.cuts(score, n, 1, 0, ratio=100, window=1).sum() > 0    # and without the histogram some pair is a cut


def test_two_cuts_closer_than_the_window_suppress_one_another():
    score, n, starts = scores("close_cuts")
    a, b = (k - 1 for k in starts)
    assert b - a == 2 and score[a, 0] < 2 * score[b, 0] and score[b, 0] < 2 * score[a, 0]
    assert sref.cuts(score, n, T, HI, ratio=200, window=4).sum() == 0                      # neither is twice the other
    assert sref.shot_ranges(sref.shot_decide(score, n, T, HI, 200, 4)) == [(0, len(score) + 1)]
    assert np.flatnonzero(sref.cuts(score, n, T, HI, ratio=200, window=1)).tolist() == [a, b]   # a window that parts them
    larger = a if score[a, 0] >= score[b, 0] else b
    assert np.flatnonzero(sref.cuts(score, n, T, HI, ratio=100, window=4)).tolist() == [larger]


def test_one_and_two_frames():
    images, _ = clips.two_shots()
    score, n = sref.shot_scores(images[:1])
    assert score.shape == (0, 2) and sref.shot_decide(score, n, T, HI).tolist() == [0]
    assert sref.shot_ranges(np.zeros(1, np.int32)) == [(0, 1)]
    k = clips.two_shots()[1][0]
    score, n = sref.shot_scores(images[k - 1:k + 1])
    assert sref.shot_decide(score, n, T, HI).tolist() == [0, 1]        # no neighbour to stand out of
    score, n = sref.shot_scores(images[:2])
    assert sref.shot_decide(score, n, T, HI).tolist() == [0, 0]


def test_equal_scores_are_cuts_with_ratio_100_only():
    n = 100
    score = np.array([[10, 0], [5000, 200], [5000, 200], [10, 0], [5000, 200]], np.int64)
    assert sref.cuts(score, n, 16, 30, ratio=100, window=4).tolist() == [0, 1, 1, 0, 1]
    assert sref.cuts(score, n, 16, 30, ratio=101, window=4).tolist() == [0, 0, 0, 0, 0]
    assert sref.cuts(score, n, 16, 30, ratio=101, window=1).tolist() == [0, 0, 0, 0, 1]
    assert sref.shot_decide(score, n, 16, 30, ratio=100).tolist() == [0, 0, 1, 2, 2, 3]
    assert sref.cuts(score, n, 51, 30, ratio=100).sum() == 0 and sref.cuts(score, n, 50, 30, ratio=100).sum() == 3
    assert sref.cuts(score, n, 50, 100, ratio=100).sum() == 3 and sref.cuts(np.array([[5000, 199]]), n, 50, 100).sum() == 0


def test_the_histogram_counts_a_moved_pixel_twice_and_blocks_are_cut_at_the_edges():
    Y = np.zeros((2, 9, 15), np.uint8)
    Y[0, 8, 14] = 200                                                  # the corner of the last block, 1 x 7 pixels
    assert sref.scores_of_planes(Y, 1).tolist() == [[200, 2]]          # no displacement finds it in the next frame
    Y[1, 7, 13] = 200                                                  # it moved by (-1, -1), into another block
    assert sref.scores_of_planes(Y, 1).tolist() == [[0, 0]]
    assert sref.scores_of_planes(Y[::-1], 1).tolist() == [[200, 0]]    # backwards (7, 14) + (1, 1) is clamped onto the pixel as well
    Y[1] = 0
    Y[1, 6, 12] = 200                                                  # by (-2, -2): outside a search of 1, inside one of 2
    assert sref.scores_of_planes(Y, 1).tolist() == [[400, 0]]          # lost by its block, and met by the block it went to
    assert sref.scores_of_planes(Y, 2).tolist() == [[0, 0]]


def test_the_default_margins_are_a_factor_of_two_on_every_clip():
    """The module docstring states what is asked of which pair."""
    for name in clips.CLIPS:
        score, n, starts = scores(name)
        A, B = score[:, 0], score[:, 1]
        for t in range(len(score)):
            what = (name, t, round(A[t] / n, 1), round(50 * B[t] / n))
            if t + 1 in starts:
                assert A[t] >= 2 * T * n and 100 * B[t] >= 2 * HI * 2 * n, what
            elif name == "flash" and t in (clips.FLASH_AT - 1, clips.FLASH_AT):
                assert 100 * A[t] < 200 * A[2 * clips.FLASH_AT - 1 - t], what
            elif name == "fast_box":
                assert 2 * 100 * B[t] <= HI * 2 * n, what
            else:
                assert 2 * A[t] <= T * n and 2 * 100 * B[t] <= HI * 2 * n, what


def test_parameter_ranges_raise():
    score = np.array([[1, 1]], np.int64)
    for bad in (dict(threshold=0), dict(threshold=256), dict(hist=-1), dict(hist=101), dict(ratio=99), dict(ratio=10001),
                dict(window=0), dict(window=17)):
        with pytest.raises(ValueError):
            sref.cuts(score, 10, **{"threshold": 16, "hist": 30, **bad})
    images = np.zeros((2, 8, 8, 3), np.float32)
    for bad in (dict(level=-1), dict(level=6), dict(search=0), dict(search=4)):
        with pytest.raises(ValueError):
            sref.shot_scores(images, **bad)


# ---- per_shot on CPU tensors --------------------------------------------------------------------------------------------------------------
def _stand_in(images, mask, scale, offset=0.0):
    """(images * scale + the mask's mean + offset, the frame index of every pixel with -1 and -2 planted)."""
    seen.append((tuple(images.shape), tuple(mask.shape)))
    n = images.shape[0]
    source = torch.arange(n, dtype=torch.int32).view(n, 1, 1).expand(n, 2, 3).clone()
    source[:, 0, 0], source[:, 1, 1] = -1, -2
    return images * scale + mask.mean() + offset, source


seen = []


def test_per_shot_slices_joins_and_offsets():
    images = torch.arange(7 * 2 * 3, dtype=torch.float32).view(7, 2, 3)
    per_frame, one, flat = torch.rand(7, 2, 3), torch.rand(1, 2, 3), torch.rand(2, 3)
    ranges = [(0, 3), (3, 4), (4, 7)]
    for mask in (per_frame, one, flat):
        seen.clear()
        out, source = shots.per_shot(_stand_in, ranges, (images, mask), 2.0, offset=1.0, frame_outputs=(1,))
        cut = mask.ndim == 3 and mask.shape[0] == 7
        assert seen == [((hi - lo, 2, 3), (hi - lo, 2, 3) if cut else tuple(mask.shape)) for lo, hi in ranges]
        want = torch.cat([images[lo:hi] * 2.0 + (mask[lo:hi] if cut else mask).mean() + 1.0 for lo, hi in ranges])
        assert torch.equal(out, want)
        assert torch.equal(source[:, 0, 1], torch.arange(7, dtype=torch.int32))          # the clip's frame numbers
        assert (source[:, 0, 0] == -1).all() and (source[:, 1, 1] == -2).all() and source.dtype == torch.int32
    # without frame_outputs nothing is offset; a single tensor comes back as one
    _, local = shots.per_shot(_stand_in, ranges, (images, one), 1.0)
    assert local[:, 0, 1].tolist() == [0, 1, 2, 0, 0, 1, 2]
    alone = shots.per_shot(lambda a: a + 1, ranges, (images,))
    assert torch.is_tensor(alone) and torch.equal(alone, images + 1)


def test_per_shot_with_one_range_is_the_function_itself():
    images, mask = torch.rand(5, 2, 3), torch.rand(5, 2, 3)
    kept = []

    def fn(a, b):
        kept.append((a, b))
        return a, b
    out = shots.per_shot(fn, [(0, 5)], (images, mask), frame_outputs=(1,))
    assert kept[0][0] is images and kept[0][1] is mask and out[0] is images and out[1] is mask


def test_ranges_are_checked_and_read_from_a_shot_tensor():
    assert shots.shot_ranges(torch.tensor([0, 0, 1, 1, 1, 2], dtype=torch.int32)) == [(0, 2), (2, 5), (5, 6)]
    assert shots.shot_ranges(torch.zeros(1, dtype=torch.int32)) == [(0, 1)]
    assert shots.clip_ranges(torch.tensor([0, 1], dtype=torch.int32), 2) == [(0, 1), (1, 2)]
    for bad in ([], [(1, 3)], [(0, 2), (3, 4)], [(0, 2), (2, 2)], [(0, 2), (1, 3)]):
        with pytest.raises(ValueError):
            shots.per_shot(lambda a: a, bad, (torch.zeros(4, 1, 1),))
    with pytest.raises(ValueError):
        shots.clip_ranges([(0, 3)], 4)
    with pytest.raises(ValueError):
        shots.shot_ranges(torch.zeros((2, 2)))


# ---- what the shot-aware fill rests on, by the temporal fill's restatement alone ------------------------------------------------------------
def test_the_plain_fill_borrows_across_the_cut_and_the_per_shot_fill_does_not():
    images, mask, ranges, whole, composed = fill_case()
    assert sref.shot_ranges(sref.detect_shots(images, T, HI)[0]) == ranges         # the detector finds that cut
    assert foreign_sources(whole[2], mask, ranges) >= 1
    assert foreign_sources(composed[2], mask, ranges) == 0
    assert (composed[2][mask >= 0.5] >= -1).all() and composed[0].shape == images.shape


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------
def test_entries_reject_bad_arguments_without_a_device(hip_lib):
    C, E, U = ctypes, _cabi.LP_E_INVALID, _cabi.LP_E_UNSUPPORTED
    side = _cabi.LP_VMASK_MAX_SIDE
    good = dict(frames=5, height=40, width=70, search=2, plane=4096, stride=40 * 70, hist=8192, score=12288)   # never dereferenced

    def measure(**change):
        return hip_lib.lp_shot_measure(C.byref(_cabi.LpShotMeasureDesc(**{**good, **change})), None)
    assert hip_lib.lp_shot_measure(None, None) == E
    for change in ({"frames": 0}, {"frames": -1}, {"height": 0}, {"height": side + 1}, {"width": 0}, {"width": side + 1}, {"search": 0},
                   {"search": _cabi.LP_SHOT_MAX_SEARCH + 1}, {"stride": 40 * 70 - 1}, {"stride": -1}, {"plane": None}, {"hist": None},
                   {"score": None}, {"hist": good["plane"]}, {"hist": good["score"]}, {"score": good["plane"]}):
        assert measure(**change) == E, change
    assert measure(frames=65536) == U
    good2 = dict(frames=5, threshold=16, hist=30, ratio=200, window=4, n_pixels=40 * 70, score=4096, shot=8192)

    def decide(**change):
        return hip_lib.lp_shot_decide(C.byref(_cabi.LpShotDecideDesc(**{**good2, **change})), None)
    assert hip_lib.lp_shot_decide(None, None) == E
    for change in ({"frames": 0}, {"threshold": 0}, {"threshold": 256}, {"hist": -1}, {"hist": 101}, {"ratio": 99}, {"ratio": 10001},
                   {"window": 0}, {"window": _cabi.LP_SHOT_MAX_WINDOW + 1}, {"n_pixels": 0}, {"n_pixels": (1 << 28) + 1},
                   {"score": None}, {"shot": None}, {"shot": good2["score"]}):
        assert decide(**change) == E, change
    assert decide(frames=65536) == U


def test_the_header_and_the_documents_say_the_shot_words():
    read = lambda *path: open(os.path.join(ROOT, *path)).read()       # noqa: E731
    header = read("include", "lanpaint_hip.h")
    assert "shot_kernel.hip" in read("lanpaint_amd", "build.py")
    for word in ("LP_SHOT_MAX_SEARCH", "LP_SHOT_MAX_WINDOW", "A[t] >= threshold * N", "100 * B[t] >= hist * 2 N", "100 * A[t] >= ratio * A[u]",
                 "dissolves, fades and wipes", "suppress one another", "cannot change a bit", "Neighbouring chunks share one frame"):
        assert word in header, word
    for doc in ("README.md", "DESIGN.md", "CHANGES.md", "INTEGRATION.md"):
        text = read(doc)
        assert "LanPaint_VideoShots" in text and "shots" in text, doc
    assert "synthetic clips only" in shots.__doc__ and "suppress one another" in shots.__doc__


# ---- the wrappers and the nodes -----------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_cpu_tensors_and_bad_arguments():
    images = torch.zeros(4, 16, 16, 3)
    for call in (lambda: shots.shot_scores(images), lambda: shots.detect_shots(images), lambda: shots.shot_scores(images.numpy()),
                 lambda: shots.shot_decide(torch.zeros((3, 2), dtype=torch.int64), 16)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for bad in (dict(level=-1), dict(level=6), dict(level=1.0), dict(search=0), dict(search=4), dict(search=True)):
        with pytest.raises(ValueError):
            shots.shot_scores(images, **bad)
    for bad in (dict(threshold=0), dict(threshold=256), dict(hist=-1), dict(hist=101), dict(ratio=99), dict(ratio=10001), dict(window=0),
                dict(window=17), dict(threshold=16.0)):
        with pytest.raises(ValueError):
            shots.detect_shots(images, **bad)
        with pytest.raises(ValueError):
            shots.shot_decide(torch.zeros((3, 2), dtype=torch.int64), 16, **bad)
    assert shots.WS_CAP_BYTES == 1 << 30 and (shots.MAX_LEVEL, shots.MAX_SEARCH, shots.MAX_WINDOW) == (5, 3, 16)
    assert (shots.THRESHOLD, shots.HIST) == (16, 30)


def test_node_protocol_mixin_and_own_mappings():
    from lanpaint_amd import propagate_nodes, stabilize_nodes, temporal_fill_checked_nodes, temporal_fill_nodes, temporal_smooth_nodes
    assert list(shots_nodes.NODE_CLASS_MAPPINGS) == list(shots_nodes.NODE_DISPLAY_NAME_MAPPINGS)
    node = shots_nodes.LanPaint_VideoShots
    req = node.INPUT_TYPES()["required"]
    assert list(req) == ["image", "threshold", "hist", "ratio", "window", "level", "search"]
    assert req["threshold"][1]["default"] == 16 and req["hist"][1]["default"] == 30 and req["window"][1]["max"] == 16
    assert all(len(v[1]["tooltip"]) > 20 for v in req.values())
    assert "suppress one another" in req["window"][1]["tooltip"] and "synthetic clips only" in req["threshold"][1]["tooltip"]
    assert node.RETURN_TYPES == ("LANPAINT_SHOTS", "INT", "STRING") and node.RETURN_NAMES == ("shots", "count", "summary")
    for word in ("hard cuts", "Dissolves, fades and wipes are not detected", "suppress one another", "0-29, 30-80"):
        assert word in node.DESCRIPTION, word
    select = shots_nodes.LanPaint_VideoShotSelect
    assert list(select.INPUT_TYPES()["required"]) == ["image", "shots", "index"] and list(select.INPUT_TYPES()["optional"]) == ["mask"]
    assert select.RETURN_TYPES == ("IMAGE", "MASK")
    parents = {"LanPaint_VideoTemporalFillShots": temporal_fill_nodes.LanPaint_VideoTemporalFill,
               "LanPaint_VideoTemporalFillCheckedShots": temporal_fill_checked_nodes.LanPaint_VideoTemporalFillChecked,
               "LanPaint_VideoTemporalSmoothShots": temporal_smooth_nodes.LanPaint_VideoTemporalSmooth,
               "LanPaint_VideoMaskStabilizeShots": stabilize_nodes.LanPaint_VideoMaskStabilize,
               "LanPaint_VideoMaskPropagateShots": propagate_nodes.LanPaint_VideoMaskPropagate}
    for name, parent in parents.items():
        cls = shots_nodes.NODE_CLASS_MAPPINGS[name]
        assert issubclass(cls, parent) and issubclass(cls, shots_nodes._PerShot) and cls.__mro__[1] is shots_nodes._PerShot
        types = cls.INPUT_TYPES()
        assert types["required"] == parent.INPUT_TYPES()["required"] and list(types["optional"]) == ["shots"]
        assert types["optional"]["shots"][0] == "LANPAINT_SHOTS" and "optional" not in parent.INPUT_TYPES()
        assert cls.RETURN_TYPES == parent.RETURN_TYPES and cls.RETURN_NAMES == parent.RETURN_NAMES and cls.FUNCTION == parent.FUNCTION
        assert getattr(cls, cls.FUNCTION) is not getattr(parent, parent.FUNCTION) and "shot" in cls.DESCRIPTION
    for name, cls in shots_nodes.NODE_CLASS_MAPPINGS.items():
        assert cls.__name__ == name and callable(getattr(cls, cls.FUNCTION)) and cls.CATEGORY in ("image", "mask")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            node().detect(torch.zeros(3, 16, 16, 3))


def test_the_mixin_calls_the_parent_once_per_range_and_joins():
    """With a stand-in parent: no device."""
    calls = []

    class Parent:
        FUNCTION = "run"

        @classmethod
        def INPUT_TYPES(s):
            return {"required": {"image": ("IMAGE", {}), "mask": ("MASK", {})}}

        def run(self, image, mask, gain=1.0):
            calls.append((image.shape[0], tuple(mask.shape)))
            return (image * gain, mask.expand(image.shape[0], *mask.shape[-2:]) + 0)

    class Child(shots_nodes._PerShot, Parent):
        def run(self, image, mask, gain=1.0, shots=None):
            return self._per_shot(shots, {"image": image, "mask": mask}, gain=gain)

    image, one, per_frame = torch.rand(5, 4, 4, 3), torch.rand(1, 4, 4), torch.rand(5, 4, 4)
    assert list(Child.INPUT_TYPES()["optional"]) == ["shots"] and "optional" not in Parent.INPUT_TYPES()
    out = Child().run(image, one, 2.0, shots=[(0, 2), (2, 5)])
    assert calls == [(2, (1, 4, 4)), (3, (1, 4, 4))] and torch.equal(out[0], image * 2.0) and out[1].shape == (5, 4, 4)
    calls.clear()
    out = Child().run(image, per_frame, shots=[(0, 1), (1, 5)])
    assert calls == [(1, (1, 4, 4)), (4, (4, 4, 4))] and torch.equal(out[1], per_frame)
    calls.clear()
    Child().run(image, per_frame)
    assert calls == [(5, (5, 4, 4))]
    with pytest.raises(ValueError):
        Child().run(image, per_frame, shots=[(0, 4)])
    sel = shots_nodes.LanPaint_VideoShotSelect().select(image, [(0, 2), (2, 5)], 1, per_frame)
    assert torch.equal(sel[0], image[2:5]) and torch.equal(sel[1], per_frame[2:5])
    sel = shots_nodes.LanPaint_VideoShotSelect().select(image, [(0, 2), (2, 5)], 0)
    assert sel[0].shape[0] == 2 and sel[1].shape == (2, 4, 4) and not sel[1].any()
    assert shots_nodes.LanPaint_VideoShotSelect().select(image, [(0, 2), (2, 5)], 0, one)[1] is one
    with pytest.raises(ValueError):
        shots_nodes.LanPaint_VideoShotSelect().select(image, [(0, 2), (2, 5)], 2)
