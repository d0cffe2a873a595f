"""The robust video temporal smooth, the parts that need no device: what follows from the rule on the restatement
(tests/temporal_smooth_robust_ref.py) as bits and counts, the median's definition on hand-written lists, the C entry's argument
checks (made before any HIP call), the wrappers' argument checks, the nodes' protocol and the no-fallback errors.  The clips are
the plain smooth's (tests/test_temporal_smooth_host.py) and two pop clips made from its pan.  Layouts, constants and names against
the header are tests/test_cabi_mirror.py's, for the whole C ABI."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi
from tests import temporal_smooth_ref as sref
from tests import temporal_smooth_robust_ref as rref
from tests.compare import _f32_bits as _bits
from tests.temporal_clips import (POP, RADII, check_ghost_removed, check_pan_equals_plain, check_pop, check_robust_noise as check_noise,
                                  check_two_frame_pop, ghost_clip, noise_clip, pop_clip, smooth_pan_clip as pan_clip,
                                  smooth_still_clip as still_clip)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- what follows from the rule, on the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", RADII)
def test_pan_with_flicker_gives_the_plain_rules_bits(radius):
    _, clip, mask = pan_clip()
    check_pan_equals_plain(rref.temporal_smooth_robust_ref(clip, mask, radius, 24), sref.temporal_smooth_ref(clip, mask, radius, 24))


@pytest.mark.parametrize("radius", RADII)
def test_a_pop_of_one_frame_is_removed_and_the_plain_rule_keeps_it(radius):
    clip, mask = pop_clip((3,))
    check_pop(rref.temporal_smooth_robust_ref(clip, mask, radius, 24), sref.temporal_smooth_ref(clip, mask, radius, 24))


@pytest.mark.parametrize("radius", RADII)
def test_a_pop_of_two_frames_is_removed_from_radius_two_on(radius):
    clip, mask = pop_clip((3, 4))
    check_two_frame_pop(radius, rref.temporal_smooth_robust_ref(clip, mask, radius, 24))


def test_a_pop_under_flicker_is_brought_down_to_the_flicker():
    clean, clip, mask = pan_clip()
    clip = clip.copy()
    clip[3][mask[3] == 1] += POP
    out, _, replaced = rref.temporal_smooth_robust_ref(clip, mask, 2, 24)
    plain = sref.temporal_smooth_ref(clip, mask, 2, 24)[0]
    worst, kept = float(np.abs(out - clean)[3].max()), float(np.abs(plain - clean)[3].max())
    print(f"largest error in the pop's frame: robust {worst:.5f}, plain {kept:.5f}")
    assert kept == 0.21875 and abs(worst - 0.01875) < 1e-6 and (replaced[3][mask[3] == 1] == 1).all()


def test_the_ghost_is_removed():
    clip, mask = ghost_clip()
    check_ghost_removed(rref.temporal_smooth_robust_ref(clip, mask, 2, 24))


@pytest.mark.parametrize("radius", RADII)
def test_noise_variance_falls_as_the_weights_say_and_nothing_is_replaced(radius):
    _, clip, mask = noise_clip()
    check_noise(radius, *rref.temporal_smooth_robust_ref(clip, mask, radius, 24))


def test_one_frame_two_frames_an_empty_mask_and_a_still_clip():
    _, clip, mask = noise_clip()
    out, support, replaced = rref.temporal_smooth_robust_ref(clip[:1], mask, 2, 24)
    assert (_bits(out) == _bits(clip[:1])).all() and (support[0] == np.where(mask == 1, 0, -1)).all() and (replaced == support).all()
    for radius in RADII:                                               # two frames: n < 3, the plain rule's bits
        out, support, replaced = rref.temporal_smooth_robust_ref(clip[:2], mask, radius, 24)
        plain = sref.temporal_smooth_ref(clip[:2], mask, radius, 24)
        assert (_bits(out) == _bits(plain[0])).all() and (support == plain[1]).all() and (replaced[:, mask == 1] == 0).all()
        assert (support > 0).any()
    out, support, replaced = rref.temporal_smooth_robust_ref(clip, np.zeros_like(mask), 2, 24)
    assert (_bits(out) == _bits(clip)).all() and (support == -1).all() and (replaced == -1).all()
    still, mask = still_clip()
    for motion in rref.MOTIONS:
        out, support, replaced = rref.temporal_smooth_robust_ref(still, mask, 3, 24, motion)
        assert (_bits(out) == _bits(still)).all() and (replaced[:, mask == 1] == 0).all()
        assert (support[4][mask == 1] == 6).all() and (support[0][mask == 1] == 3).all() and (support[7][mask == 1] == 4).all()
    negative = -still                                                  # -x + 0 / W keeps the sign bit of every value too
    out, _, _ = rref.temporal_smooth_robust_ref(negative, mask, 2, 0)
    assert (_bits(out) == _bits(negative)).all()


def test_a_rejected_sample_does_not_end_the_chain():
    """The still clip with one frame replaced under the mask, on fields that are zero (a matcher sees the frame and answers with
    vectors that leave the plane): its neighbours walk through it and keep every other sample."""
    from tests import propagate_ref as ref
    from tests import temporal_fill_ref as tref
    still, mask = still_clip()
    clip = still.copy()
    clip[4][mask == 1] = 1.0
    known = tref.known_bits(mask, clip.shape[0])
    zero = np.zeros((clip.shape[0], *ref.grid_of(*mask.shape), 2), np.int64)
    out, support, replaced = rref.robust_frames(clip, known, zero, zero, 3, 24)
    assert (_bits(out) == _bits(still)).all() and (replaced[4][mask == 1] == 1).all() and int((replaced == 1).sum()) == int(mask.sum())
    assert (support[3][mask == 1] == 5).all() and (support[4][mask == 1] == 6).all() and (support[1][mask == 1] == 3).all()
    plain = sref.smooth_frames(clip, known, zero, zero, 3, 24)[1]
    assert (plain[3][mask == 1] == 3).all()                            # the plain chain ends at the frame


# ---- the median ---------------------------------------------------------------------------------------------------------------------------
def test_the_median_on_hand_written_lists():
    cases = [([10], [0], 0), ([10, 200], [0, 1], 0), ([200, 10], [0, 3], 0),                 # n < 3: the own pixel
             ([10, 20, 30], [0, 1, 2], 1), ([30, 20, 10], [0, 1, 2], 1), ([20, 30, 10], [0, 1, 3], 0),
             ([10, 20, 30, 40], [0, 1, 2, 3], 1), ([40, 30, 20, 10], [0, 1, 2, 3], 2),       # even n: the lower of the middle two
             ([5, 5, 5], [0, 1, 2], 1), ([5, 5, 5, 5], [0, 1, 3, 4], 1), ([7, 5, 5, 9, 5], [0, 1, 2, 3, 4], 4),   # ties: the walk's order
             ([9, 5, 9, 5, 9], [0, 1, 2, 3, 4], 0), ([255, 0, 0, 255, 255], [0, 2, 3, 5, 6], 0),
             (list(range(17)), list(range(17)), 8), (list(range(16, -1, -1)), list(range(17)), 8), ([3] * 17, list(range(17)), 8)]
    for lumas, orders, want in cases:
        assert rref.median_index(lumas, orders) == want, (lumas, orders)
        slots = 17
        exists = np.zeros((1, slots), bool)
        s = np.zeros((1, slots, 1), np.float32)
        exists[0, orders] = True
        s[0, orders, 0] = np.float32(lumas) / np.float32(255)         # one channel: the luma is the code
        assert (rref.luma_of(s)[0, orders] == lumas).all()
        assert rref.reference_index(exists, s)[0] == want, (lumas, orders)
    rng = np.random.default_rng(12)                                    # and the two forms of the restatement on random lists
    for _ in range(300):
        slots = int(rng.integers(3, 18))
        exists = rng.random((1, slots)) < 0.7
        exists[0, 0] = True
        s = (rng.integers(0, 6, (1, slots, 1)) * 50 / 255).astype(np.float32)
        orders = np.nonzero(exists[0])[0].tolist()
        assert rref.reference_index(exists, s)[0] == rref.median_index(rref.luma_of(s)[0, orders].tolist(), orders)


def test_the_luma_is_the_propagate_sections():
    from tests import propagate_ref as ref
    images = np.random.default_rng(13).random((2, 5, 6, 4)).astype(np.float32) * 1.4 - 0.2
    for channels in (1, 2, 3, 4):
        assert (rref.luma_of(images[..., :channels]) == ref.luma(images[..., :channels])).all()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_entry_rejects_bad_arguments_without_a_device(hip_lib):
    C, E, U = ctypes, _cabi.LP_E_INVALID, _cabi.LP_E_UNSUPPORTED
    side = _cabi.LP_VMASK_MAX_SIDE
    a = [C.c_void_p(4096 * (i + 1)) for i in range(8)]                # never dereferenced: validation comes before any HIP call
    names = [f for f, t in _cabi.LpTsmoothRobustDesc._fields_ if t is C.c_void_p]
    assert names == ["fwd", "bwd", "known", "images", "out", "support", "replaced"]
    # frames 3 .. 5 of 10 with radius 2: fwd of 3 .. 6, bwd of 2 .. 5
    good = dict(frames=10, height=40, width=70, channels=3, first=3, count=3, radius=2, tolerance=24, fwd_first=3, fwd_count=4,
                bwd_first=2, bwd_count=4, known_stride=40 * 70, **dict(zip(names, a)))

    def call(**change):
        return hip_lib.lp_tsmooth_robust(C.byref(_cabi.LpTsmoothRobustDesc(**{**good, **change})), None)
    assert hip_lib.lp_tsmooth_robust(None, None) == E
    for change in ({"frames": 0}, {"frames": -1}, {"height": 0}, {"height": side + 1}, {"width": 0}, {"width": side + 1},
                   {"channels": 0}, {"channels": _cabi.LP_DETAIL_MAX_CHANNELS + 1}, {"radius": 0}, {"radius": _cabi.LP_TSMOOTH_MAX_RADIUS + 1},
                   {"tolerance": -1}, {"tolerance": 256}, {"first": -1}, {"first": 10}, {"count": 0}, {"count": 8}, {"count": -1},
                   {"fwd_first": 4}, {"fwd_first": -1}, {"fwd_count": 3}, {"fwd_count": 0}, {"bwd_first": 3}, {"bwd_first": -1},
                   {"bwd_count": 3}, {"bwd_count": 0}, {"known_stride": 40 * 70 - 1}, {"known_stride": -1}, {"radius": 3}):
        assert call(**change) == E, change
    for name in names:
        assert call(**{name: None}) == E, name
    for out in ("out", "support", "replaced"):                         # an output that is an input or another output
        for other in names:
            if other != out:
                assert call(**{out: good[other]}) == E, (out, other)
    assert call(frames=65536) == U


def test_the_robust_descriptor_is_the_plain_one_plus_replaced():
    py, plain = _cabi.LpTsmoothRobustDesc, _cabi.LpTsmoothDesc
    assert py._fields_[:-1] == plain._fields_ and py._fields_[-1] == ("replaced", ctypes.c_void_p)
    assert [getattr(py, f).offset for f, _ in plain._fields_] == [getattr(plain, f).offset for f, _ in plain._fields_]


def test_the_header_and_the_documents_say_the_robust_words():
    read = lambda *path: open(os.path.join(ROOT, *path)).read()       # noqa: E731
    header = read("include", "lanpaint_hip.h")
    assert 'extern "C" int lp_tsmooth_robust(' in read("lanpaint_amd", "csrc", "temporal_smooth_kernel.hip")   # beside its kernels
    assert header.index("Robust video temporal smooth") > header.index("LP_API int lp_tsmooth(")      # the section stands behind the plain one
    for word in ("LP_TSMOOTH_ROBUST_QUORUM", "lower median", "(n - 1) >> 1", "ties broken by the walk's order", "does NOT end at a sample",
                 "two witnesses overrule", "replaced = 1", "replaced = -1", "keeps x bit for bit", "R frames or fewer", "n < 3",
                 "a clip of two frames", "for every chunking", "a single outlier frame"):
        assert word in header, word
    for doc in ("README.md", "DESIGN.md", "CHANGES.md", "INTEGRATION.md"):
        text = read(doc)
        for name in ("LanPaint_VideoTemporalSmoothRobust", "temporal_smooth_robust", "lp_tsmooth_robust"):
            assert name in text, (doc, name)
    design = read("DESIGN.md")
    for word in ("VGPR", "scratch 0", "lp_tsmooth_kernel"):
        assert word in design, word
    assert re.search(r"VideoTemporalSmoothRobust\s*->\s*(LanPaint_)?MultibandBlend", read("INTEGRATION.md"))
    from lanpaint_amd import temporal_smooth, temporal_smooth_nodes
    assert "temporal_smooth_robust" in temporal_smooth.__doc__ and "a single outlier frame" in temporal_smooth.__doc__
    assert "LanPaint_VideoTemporalSmoothRobust" in temporal_smooth_nodes.LanPaint_VideoTemporalSmooth.DESCRIPTION


# ---- the wrappers and the nodes ---------------------------------------------------------------------------------------------------------
def test_temporal_smooth_robust_refuses_cpu_tensors_and_bad_arguments():
    from lanpaint_amd import shots, temporal_smooth as ts, temporal_smooth_robust as tr
    images, mask = torch.zeros(4, 16, 16, 3), torch.zeros(4, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.temporal_smooth_robust(images, mask)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.temporal_smooth_robust(images.numpy(), mask)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        shots.temporal_smooth_robust_shots(images, mask, [(0, 2), (2, 4)])
    with pytest.raises(ValueError):
        shots.temporal_smooth_robust_shots(images, mask, [(0, 3)])
    fields = torch.zeros(3, 2, 2, 2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.robust_frames(fields, fields, torch.zeros(4, 16, 16, dtype=torch.uint8), images)
    # the numbers are checked before the tensors are looked at
    for bad in (dict(radius=0), dict(radius=9), dict(radius=2.0), dict(radius=True), dict(tolerance=-1), dict(tolerance=256),
                dict(tolerance=24.0), dict(motion="subject"), dict(motion=None), dict(levels=0), dict(levels=7), dict(search=0),
                dict(search=8), dict(smooth=-1), dict(smooth=65)):
        with pytest.raises(ValueError):
            tr.temporal_smooth_robust(images, mask, **bad)
    for bad in (dict(radius=0), dict(radius=9), dict(tolerance=-1), dict(tolerance=256)):
        with pytest.raises(ValueError):
            tr.robust_frames(fields, fields, torch.zeros(4, 16, 16, dtype=torch.uint8), images, **bad)
    assert tr.QUORUM == 2 and not hasattr(tr, "WS_CAP_BYTES") and ts.WS_CAP_BYTES == 1 << 30     # one cap for both forms
    import inspect
    assert list(inspect.signature(tr.robust_frames).parameters) == list(inspect.signature(ts.smooth_frames).parameters) + ["replaced"]
    assert list(inspect.signature(tr.temporal_smooth_robust).parameters) == list(inspect.signature(ts.temporal_smooth).parameters)


def test_node_protocol_and_own_mappings():
    from lanpaint_amd import shots_nodes, temporal_smooth_nodes, temporal_smooth_robust_nodes as mod
    node, per_shot = mod.LanPaint_VideoTemporalSmoothRobust, mod.LanPaint_VideoTemporalSmoothRobustShots
    assert mod.NODE_CLASS_MAPPINGS == {"LanPaint_VideoTemporalSmoothRobust": node, "LanPaint_VideoTemporalSmoothRobustShots": per_shot}
    assert list(mod.NODE_DISPLAY_NAME_MAPPINGS) == list(mod.NODE_CLASS_MAPPINGS)
    assert list(temporal_smooth_nodes.NODE_CLASS_MAPPINGS) == ["LanPaint_VideoTemporalSmooth"] and len(shots_nodes.NODE_CLASS_MAPPINGS) == 7
    types, plain = node.INPUT_TYPES(), temporal_smooth_nodes.LanPaint_VideoTemporalSmooth.INPUT_TYPES()
    assert list(types) == ["required"] and list(types["required"]) == list(plain["required"])
    for name, spec in types["required"].items():                       # the plain node's inputs: types, defaults and ranges
        theirs = plain["required"][name]
        assert spec[0] == theirs[0] and {k: v for k, v in spec[1].items() if k != "tooltip"} == {k: v for k, v in theirs[1].items() if k != "tooltip"}
        assert len(spec[1]["tooltip"]) > 20, name
    assert "longest outlier" in types["required"]["radius"][1]["tooltip"] and "median" in types["required"]["tolerance"][1]["tooltip"]
    assert plain == temporal_smooth_nodes.LanPaint_VideoTemporalSmooth.INPUT_TYPES()      # and the plain node's are not touched
    for word in ("boiling", "outlier", "median", "tolerance", "multiband blend", "grain", "in place of the plain temporal smooth",
                 "longest outlier removed", "`radius` frames or fewer", "removed on purpose", "support", "replaced", "decode", "stitch"):
        assert word in node.DESCRIPTION, word
    assert node.RETURN_TYPES == ("IMAGE", "MASK", "MASK") and node.RETURN_NAMES == ("image", "support", "replaced")
    assert node.FUNCTION == "smooth" and callable(getattr(node, node.FUNCTION)) and node.CATEGORY == "image"
    assert issubclass(per_shot, node) and per_shot.__mro__[1] is shots_nodes._PerShot and "shot" in per_shot.DESCRIPTION
    types = per_shot.INPUT_TYPES()
    assert types["required"] == node.INPUT_TYPES()["required"] and list(types["optional"]) == ["shots"]
    assert per_shot.RETURN_TYPES == node.RETURN_TYPES and per_shot.RETURN_NAMES == node.RETURN_NAMES and per_shot.FUNCTION == node.FUNCTION
    assert per_shot.smooth is not node.smooth
    for name, cls in mod.NODE_CLASS_MAPPINGS.items():
        assert cls.__name__ == name
    if not torch.cuda.is_available():
        for cls in (node, per_shot):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                cls().smooth(torch.zeros(3, 16, 16, 3), torch.zeros(3, 16, 16))
