"""Clips of tens of frames for the temporal fill, the checked fill and the temporal smooth: plain numpy, no device.  The short
clips of the other test modules end before an origin is older than 4 frames, a smooth chain longer than 4 steps or a call has more
than 32 steps; these are built so that all of that happens, and tests/test_temporal_long_clips_host.py asserts that it does.
Below them, the clips, cases and checks that the host tests of the temporal fill, the checked fill, the smooth and the robust
smooth share with their device twins: numpy and the restatements only."""
import functools

import numpy as np

from tests import propagate_ref as ref
from tests import temporal_fill_checked_ref as cref
from tests import temporal_fill_ref as tref
from tests import temporal_smooth_ref as sref
from tests import temporal_smooth_robust_ref as rref
from tests.compare import _f32_bits
from tests.inputs import _rng, _video, _wild_video

BOX = (8, 10)                          # the subject that stays: rows x columns, at (H // 3, W // 3)
CORNER = 5                             # the side of the box in the bottom-left corner of every other frame


@functools.lru_cache(maxsize=None)
def drift_clip(F, H, W, C=3, every=4, noise=0.01, seed=0):
    """fp32 [F, H, W, C]: frames cut from one random canvas of H x (W + (F - 1) // every + 1); the cut moves one whole pixel in x
    every `every` frames, and every frame has Gaussian noise of `noise` of its own.  Do not write to the result: it is shared."""
    rng = np.random.default_rng([F, H, W, C, every, seed, 21])
    canvas = rng.random((H, W + (F - 1) // every + 1, C), dtype=np.float32)
    frames = np.stack([canvas[:, t // every:t // every + W] for t in range(F)])
    clip = (frames + rng.normal(0, noise, frames.shape)).astype(np.float32)
    clip.setflags(write=False)
    return clip


def box_of(H, W):
    """The big box's (y, x)."""
    return H // 3, W // 3


def stay_then_leave_mask(F, H, W, first, last):
    """fp32 [F, H, W]: an 8 x 10 box at (H // 3, W // 3) in the frames first .. last - 1; in every other frame a 5 x 5 box in the
    bottom-left corner, so that no frame has an empty mask."""
    mask = np.zeros((F, H, W), np.float32)
    y, x = box_of(H, W)
    for t in range(F):
        if first <= t < last:
            mask[t, y:y + BOX[0], x:x + BOX[1]] = 1
        else:
            mask[t, H - CORNER:, :CORNER] = 1
    return mask


def random_mask(F, H, W, share=0.3, seed=0):
    """fp32 [F, H, W]: every pixel of every frame is masked with probability `share`, on its own."""
    return (np.random.default_rng([F, H, W, seed, 22]).random((F, H, W)) < share).astype(np.float32)


def scene_change(images, frame, amount=0.35, width=3, margin=6):
    """A copy of `images` in which, from `frame` on, `amount` is added to a patch over the `width` left columns of the big box and
    the known pixels `margin` beside, above and below them.  The forward witness of the checked fill comes from before `frame`
    and the backward witness from after it, so they differ there by 89 grey levels, of which the rule forgives a bias of 32."""
    F, H, W = images.shape[:3]
    y, x = box_of(H, W)
    out = np.array(images, dtype=np.float32)
    out[frame:, max(y - margin, 0):y + BOX[0] + margin, max(x - margin, 0):x + width] += np.float32(amount)
    return out


CHECKED_FRAMES = 5                                                                  # the stage case: frame 2 of 5, its donor frame 3


@functools.lru_cache(maxsize=None)
def second_object_clip():
    """(boxless clip, clip, mask): 10 frames of 64 x 96 x 3 on one still random canvas; a second object, a 40 x 40 texture, moves
    2 px per frame down through the path of a 12 x 12 constant box that moves 5 px per frame to the right on top of it; the mask
    is the box grown by 1.  The one-layer background field cannot hold both motions."""
    frames, H, W = 10, 64, 96
    rng = np.random.default_rng(11)
    clean = np.repeat(rng.random((1, H, W, 3), dtype=np.float32), frames, axis=0)
    tex = rng.random((40, 40, 3), dtype=np.float32)
    for t in range(frames):
        clean[t, 2 * t:2 * t + 40, 36:76] = tex
    clip, mask = clean.copy(), np.zeros((frames, H, W), np.float32)
    for t in range(frames):
        y, x = 26, 6 + 5 * t
        clip[t, y:y + 12, x:x + 12] = 0.5
        mask[t, y - 1:y + 13, x - 1:x + 13] = 1
    return clean, clip, mask


# what the restatements give on it at the defaults and agree = 8; the conditions these satisfy are in the test below
SECOND_OBJECT = dict(masked=1960, plain_wrong=556, filled=1169, wrong=67, disputed=791, verified=343, verified_wrong=14)


def second_object_counts(plain, checked):
    """The counts of SECOND_OBJECT from the outputs of the plain and the checked call on the clip.  Wrong: a borrowed pixel whose
    bits differ from the clip drawn without the box."""
    clean, _, mask = second_object_clip()
    m = mask == 1
    (pf, _, ps), (cf, cr, cs, cw) = plain, checked
    plain_wrong = (_f32_bits(pf) != _f32_bits(clean)).any(-1) & m & (ps >= 0)
    wrong = (_f32_bits(cf) != _f32_bits(clean)).any(-1) & m & (cs >= 0)
    assert ((cr == 1) == (m & (cs < 0))).all(), "((cr == 1) == (m & (cs < 0))).all()"
    return dict(masked=int(m.sum()), plain_wrong=int(plain_wrong.sum()), filled=int((m & (cs >= 0)).sum()), wrong=int(wrong.sum()),
                disputed=int((cs == cref.DISPUTED).sum()), verified=int((cw == 2).sum()), verified_wrong=int((wrong & (cw == 2)).sum()))


@functools.lru_cache(maxsize=None)
def fill_pan_clip():
    """(boxless clip, clip, mask): 8 frames of 48 x 64 x 3 cut from one random canvas, panning (1, -2) px per frame; a 12 x 12
    constant box moves 5 px per frame across it; the mask is the box grown by 1."""
    rng = np.random.default_rng(5)
    F, H, W = 8, 48, 64
    canvas = rng.random((H + F, W + 2 * F, 3), dtype=np.float32)
    clean = np.stack([canvas[t:t + H, 2 * (F - 1 - t):2 * (F - 1 - t) + W] for t in range(F)])
    clip, mask = clean.copy(), np.zeros((F, H, W), np.float32)
    for t in range(F):
        y, x = 18, 4 + 5 * t
        clip[t, y:y + 12, x:x + 12] = 0.5
        mask[t, y - 1:y + 13, x - 1:x + 13] = 1
    return clean, clip, mask


@functools.lru_cache(maxsize=None)
def fill_still_clip(step):
    """(still canvas, clip, mask): 8 equal frames of 32 x 48 x 3 with an 8 x 8 constant box that moves `step` px per frame."""
    F, H, W = 8, 32, 48
    still = np.repeat(np.random.default_rng(6).random((1, H, W, 3), dtype=np.float32), F, axis=0)
    clip, mask = still.copy(), np.zeros((F, H, W), np.float32)
    for t in range(F):
        clip[t, 12:20, 10 + step * t:18 + step * t] = 0.25
        mask[t, 12:20, 10 + step * t:18 + step * t] = 1
    return still, clip, mask


@functools.lru_cache(maxsize=None)
def clean_clip(name, noisy):
    """(clip, mask) of `pan_clip()` or `still_clip(2)`, with Gaussian noise of sigma 4 grey levels on every frame when `noisy`."""
    _, clip, mask = fill_pan_clip() if name == "pan" else fill_still_clip(2)
    if noisy:
        clip = (clip + np.random.default_rng(3).normal(0, 4 / 255, clip.shape)).astype(np.float32)
    return clip, mask


CLEAN_CLIPS = [("pan", False), ("still", False), ("pan", True), ("still", True)]


@functools.lru_cache(maxsize=None)
def random_clip():
    """A random moving video of 5 x 40 x 70 x 3 under random masks: every pixel class, disputes included."""
    images = _video(CHECKED_FRAMES, 40, 70)
    mask = (_rng(CHECKED_FRAMES, 40, 70, 0, 5).random((CHECKED_FRAMES, 40, 70)) < 0.3).astype(np.float32)
    return images, mask


def check_invariant(images, plain, checked, what):
    """What follows from the rule, between a plain and a checked result on the same arguments."""
    (pf, pr, ps), (cf, cr, cs, cw) = plain, checked
    agreed, nan = cs != cref.DISPUTED, np.isnan(pf)
    assert (cs[agreed] == ps[agreed]).all() and (_f32_bits(cr)[agreed] == _f32_bits(pr)[agreed]).all(), what
    assert (((_f32_bits(cf) == _f32_bits(pf)) | (nan & np.isnan(cf)))[agreed]).all(), what
    assert (ps[~agreed] >= 0).all(), what
    assert ((_f32_bits(cf) == _f32_bits(images)) | np.isnan(images))[~agreed].all(), what
    masked = pr.astype(bool) | (ps != np.arange(len(ps))[:, None, None])          # the plain call's mask bits
    assert ((cr == 1) == (masked & (cs < 0))).all() and ((cr == 0) | (cr == 1)).all(), what
    assert (cw[~masked] == 0).all() and (cw[cs < 0] == 0).all() and ((cw >= 1) == (masked & (cs >= 0))).all() and cw.max() <= 2, what


@functools.lru_cache(maxsize=None)
def pair_case(H, W, wild=False, C=3):
    """Frame 2 of 5 with its donor 3: random known bits of both, of the frame a quarter to three quarters by block, a random field of up to 2.5 pixels, a random state of the donor
    with origins in every frame, a random forward `source` under the mask and a forward `filled` that is, block by block, the
    backward sample itself, that sample darker or brighter by 0.3 or by 0.05, or noise.
    (images, vec, known [2, H, W], org, pos, source_t, filled_t)."""
    rng = _rng(H, W, int(wild), C, 8)
    images = (_wild_video if wild else _video)(CHECKED_FRAMES, H, W, C)
    gh, gw = ref.grid_of(H, W)
    vec = rng.integers(-40, 41, (gh, gw, 2)).astype(np.int32)
    share = cref.per_pixel(rng.choice([0.25, 0.5, 0.75], (gh, gw)), H, W)   # so that a block holds few or many pixels to compare
    known = (rng.random((2, H, W)) < np.stack([share, np.full((H, W), 0.5)])).astype(np.uint8)
    org = rng.integers(-1, CHECKED_FRAMES, (H, W)).astype(np.int32)
    pos = np.stack([rng.integers(-40, 16 * H + 40, (H, W)), rng.integers(-40, 16 * W + 40, (H, W))], axis=-1).astype(np.int32)
    source = np.where(known[0] != 0, 2, rng.choice([-1, 0, 1, 3, 4], (H, W))).astype(np.int32)
    b_org, b_pos = tref.carry(2, known[0], 3, known[1], vec, (org, pos), 0)
    has_b = (known[0] == 0) & (b_org >= 0)
    filled = images[2].copy()
    filled[has_b] = tref.sample(images, b_org[has_b], b_pos[has_b][:, 0], b_pos[has_b][:, 1])
    mode = cref.per_pixel(rng.integers(0, 5, (gh, gw)), H, W)
    with np.errstate(invalid="ignore"):
        filled = filled + np.choose(mode, [0, -0.3, 0.3, 0, 0.05]).astype(np.float32)[..., None] + rng.normal(0, 0.004, filled.shape)
    filled = np.where((mode == 3)[..., None], rng.random(filled.shape), filled).astype(np.float32)
    filled = np.where((known[0] != 0)[..., None], images[2], filled)
    return images, vec, known, org, pos, source, filled


def pair_want(case, state, reach, agree, stats=None):
    """What the step must leave for `case`: the state (org, pos) and frame 2's (filled, source, remaining, witnesses)."""
    images, vec, known, org, pos, source, filled = case
    b_org, b_pos = tref.carry(2, known[0], 3, known[1], vec, (org, pos) if state else None, reach)
    remaining = ((known[0] == 0) & (source == -1)).astype(np.float32)
    return (b_org, b_pos), cref.pair(2, known[0], images, b_org, b_pos, filled, source, remaining, agree, stats)


def check_clean(plain, checked):
    assert not (checked[2] == cref.DISPUTED).any() and (checked[3] == 2).any(), "no disputed pixel and some pixel with two witnesses"
    for p, c in zip(plain, checked):
        assert (_f32_bits(p) == _f32_bits(c)).all() if p.dtype == np.float32 else (p == c).all(), (
            "the plain fill's output against the checked fill's")


STILL_REMAINING = {1: 288, 2: 96, 8: 0}                               # reach -> pixels no frame within it shows


def check_fill_pan(filled, remaining, source):
    clean, clip, mask = fill_pan_clip()
    assert int(mask.sum()) == 1568 and not remaining.any(), "int(mask.sum()) == 1568 and not remaining.any()"
    assert (_f32_bits(filled) == _f32_bits(clean)).all(), "filled against the clean clip"  # all 1568 masked pixels are the true background, bit for bit
    assert ((source >= 0) & (source < 8)).all() and ((source == np.arange(8)[:, None, None]) == (mask == 0)).all(), (
        "every source in the clip, a frame's own index exactly outside the mask")


def check_fill_still(reach, filled, remaining, source):
    still, clip, mask = fill_still_clip(2)
    assert int(remaining.sum()) == STILL_REMAINING[reach], "int(remaining.sum()) == STILL_REMAINING[reach]"
    assert ((remaining == 1) == ((mask == 1) & (source == -1))).all(), "((remaining == 1) == ((mask == 1) & (source == -1))).all()"
    age = np.abs(source - np.arange(8)[:, None, None])
    assert (age[source >= 0] <= reach).all(), "(age[source >= 0] <= reach).all()"
    assert (_f32_bits(filled) == np.where((remaining == 1)[..., None], _f32_bits(clip), _f32_bits(still))).all(), (
        "filled: the clip where the hole remains, the still frame elsewhere")


def check_fill_fixed(filled, remaining, source):
    _, clip, mask = fill_still_clip(0)
    assert (_f32_bits(remaining) == _f32_bits(mask)).all() and (_f32_bits(filled) == _f32_bits(clip)).all(), (
        "remaining against the mask and filled against the clip, bit for bit")
    assert (source == np.where(mask == 1, -1, np.arange(8)[:, None, None])).all(), (
        "source: -1 under the mask, the frame's own index outside")


LONG_FRAMES, LONG_PLANE = 48, (23, 33)
LONG_LEVELS, LONG_SEARCH, LONG_SMOOTH = 3, 2, 8
LONG_LEAVES = 40                                                            # the big box is in the frames .. LEAVES - 1
LONG_ARRIVES = 6                                                            # the checked clip: the big box is in ARRIVES .. LEAVES - 1
LONG_CHANGE = 30                                                            # the checked clip: the scene changes in this frame
LONG_SMOOTH_FRAMES = 20


def long_fill_clip(one_mask=False):
    """(images, mask): the drift clip, the big box until it leaves in frame LEAVES; `one_mask`: the big box in every frame."""
    mask = stay_then_leave_mask(LONG_FRAMES, *LONG_PLANE, 0, LONG_LEAVES)
    return drift_clip(LONG_FRAMES, *LONG_PLANE), mask[0] if one_mask else mask


@functools.lru_cache(maxsize=None)
def long_fill_want(reach, one_mask=False):
    return tref.temporal_fill_ref(*long_fill_clip(one_mask), LONG_LEVELS, LONG_SEARCH, LONG_SMOOTH, reach)


@functools.lru_cache(maxsize=None)
def long_checked_clip(one_mask=False):
    """(images, mask): the drift clip with a scene change in frame CHANGE, the big box in the frames ARRIVES .. LEAVES - 1."""
    mask = stay_then_leave_mask(LONG_FRAMES, *LONG_PLANE, LONG_ARRIVES, LONG_LEAVES)
    images = scene_change(drift_clip(LONG_FRAMES, *LONG_PLANE), LONG_CHANGE)
    images.setflags(write=False)
    return images, mask[LONG_ARRIVES] if one_mask else mask


@functools.lru_cache(maxsize=None)
def long_checked_want(reach, agree, one_mask=False):
    return cref.temporal_fill_checked_ref(*long_checked_clip(one_mask), LONG_LEVELS, LONG_SEARCH, LONG_SMOOTH, reach, agree)


def long_smooth_clip(frames, channels=3, one_mask=False):
    """(images, mask): the first `frames` frames of the drift clip under a random mask of 30 %."""
    mask = random_mask(frames, *LONG_PLANE)
    return drift_clip(LONG_FRAMES, *LONG_PLANE, channels)[:frames], mask[0] if one_mask else mask


@functools.lru_cache(maxsize=None)
def _long_smooth_fields(frames, motion, channels, one_mask):
    images, mask = long_smooth_clip(frames, channels, one_mask)
    known = tref.known_bits(mask, frames)
    return known, sref.fields(images, known, motion, LONG_LEVELS, LONG_SEARCH, LONG_SMOOTH)


@functools.lru_cache(maxsize=None)
def long_smooth_want(frames, radius, tolerance, motion, channels=3, one_mask=False):
    """`sref.temporal_smooth_ref` of the case, its two lines with the fields -- which know nothing of radius and tolerance --
    computed once (test_the_shared_fields_give_the_whole_restatement)."""
    known, (fwd, bwd) = _long_smooth_fields(frames, motion, channels, one_mask)
    return sref.smooth_frames(long_smooth_clip(frames, channels, one_mask)[0], known, fwd, bwd, radius, tolerance)


RADII = (1, 2, 3)
PAN_PIXELS = {1: 1344, 2: 896, 3: 448}                               # masked pixels of the frames R .. F - 1 - R: 224 a frame
NOISE_RATIO = {1: 6 / 16, 2: 70 / 256, 3: 924 / 4096}                # sum w^2 / (sum w)^2: 0.375, 0.273, 0.226


@functools.lru_cache(maxsize=None)
def smooth_pan_clip():
    """(clean clip, flickering clip, mask): 8 frames of 48 x 64 x 3 cut from one canvas of 8-bit values, panning (1, -2) px per
    frame; the mask is fixed to the canvas, and under it even frames are 8 / 256 too bright and odd frames as much too dark."""
    rng = np.random.default_rng(6)
    F, H, W = 8, 48, 64
    canvas = (rng.integers(64, 192, (H + F, W + 2 * F, 3)) / 256).astype(np.float32)
    cm = np.zeros((H + F, W + 2 * F), np.float32)
    cm[26:40, 30:46] = 1

    def cut(a, t):
        return a[t:t + H, 2 * (F - 1 - t):2 * (F - 1 - t) + W]
    clean = np.stack([cut(canvas, t) for t in range(F)])
    mask = np.stack([cut(cm, t) for t in range(F)])
    clip = clean.copy()
    for t in range(F):
        clip[t][mask[t] == 1] += np.float32(8 / 256 if t % 2 == 0 else -8 / 256)
    return clean, clip, mask


@functools.lru_cache(maxsize=None)
def smooth_still_clip():
    """(still clip, mask): 9 equal frames of 32 x 48 x 3 in 0.25 .. 0.75 and a static mask."""
    F, H, W = 9, 32, 48
    frame = (0.25 + 0.5 * np.random.default_rng(7).random((1, H, W, 3))).astype(np.float32)
    mask = np.zeros((H, W), np.float32)
    mask[10:22, 14:34] = 1
    return np.repeat(frame, F, axis=0), mask


@functools.lru_cache(maxsize=None)
def noise_clip():
    """(still clip, noisy clip, mask): iid normal noise of sigma 0.02 under the mask of the still clip."""
    still, mask = smooth_still_clip()
    clip = still.copy()
    clip[:, mask == 1] += np.random.default_rng(8).normal(0, 0.02, (still.shape[0], int(mask.sum()), 3)).astype(np.float32)
    return still, clip, mask


GHOST_FRAME, GHOST = 4, (slice(13, 19), slice(20, 28))               # a 6 x 8 patch inside the hole


@functools.lru_cache(maxsize=None)
def ghost_clip():
    """(clip, mask): the still clip with a patch of 1.0 in one frame, inside the hole: at least 64 grey levels from the canvas."""
    still, mask = smooth_still_clip()
    clip = still.copy()
    clip[GHOST_FRAME][GHOST] = 1.0
    return clip, mask


def check_outside(images, mask, out, support):
    """Everything outside the mask is bits of the input with support -1; under it support counts 0 .. 2R."""
    under = np.broadcast_to(mask == 1, support.shape)
    assert (_f32_bits(out)[~under] == _f32_bits(images)[~under]).all() and (support[~under] == -1).all() and (support[under] >= 0).all(), (
        "outside the mask: the input's bits and support -1; under it: support >= 0")


def check_smooth_pan(radius, motion, out, support):
    clean, clip, mask = smooth_pan_clip()
    F = clip.shape[0]
    under = mask == 1
    assert (np.abs(clip - clean)[under] == np.float32(8 / 256)).all(), "the clip's error under the mask"  # the error of the input, everywhere under the mask
    check_outside(clip, mask, out, support)
    inner = np.zeros_like(under)
    inner[radius:F - radius] = under[radius:F - radius]
    assert int(inner.sum()) == PAN_PIXELS[radius], "int(inner.sum()) == PAN_PIXELS[radius]"
    if motion == "background":
        assert (_f32_bits(out)[inner] == _f32_bits(clean)[inner]).all(), "out against the clean clip in the interior"  # every one of them is the clean canvas, bit for bit
        assert (support[inner] == 2 * radius).all(), "(support[inner] == 2 * radius).all()"
    else:
        assert np.abs(out - clean)[under].mean() < np.abs(clip - clean)[under].mean(), (
            "the mean error under the mask after smoothing against before")


def check_smooth_noise(radius, out, support):
    still, clip, mask = noise_clip()
    F = clip.shape[0]
    check_outside(clip, mask, out, support)
    inner = slice(radius, F - radius)
    before, after = (clip - still)[inner][:, mask == 1], (out - still)[inner][:, mask == 1]
    ratio = float(after.astype(np.float64).var() / before.astype(np.float64).var())
    print(f"radius {radius}: variance ratio {ratio:.4f}, the weights give {NOISE_RATIO[radius]:.4f}")
    assert abs(ratio / NOISE_RATIO[radius] - 1) <= 0.15, (radius, ratio)


def check_smooth_ghost(out, support):
    clip, mask = ghost_clip()
    check_outside(clip, mask, out, support)
    for t in range(GHOST_FRAME - 2, GHOST_FRAME + 3):                  # the patch's frame and its four neighbours
        assert (_f32_bits(out[t][GHOST]) == _f32_bits(clip[t][GHOST])).all(), t
    assert (support[GHOST_FRAME][GHOST] == 0).all(), "(support[GHOST_FRAME][GHOST] == 0).all()"
    assert (support[GHOST_FRAME - 1][GHOST] == 2).all() and (support[GHOST_FRAME + 2][GHOST] == 3).all(), (
        "the support beside the ghost frame")   # the chain ends at the patch
    assert (_f32_bits(out) == _f32_bits(clip)).all(), "out against the clip"                           # and the rest of the clip is still


POP = np.float32(64 / 256)


@functools.lru_cache(maxsize=None)
def pop_clip(frames):
    """(clip, mask): the clean pan clip with 64 / 256 added under the mask of the frames `frames`."""
    clean, _, mask = smooth_pan_clip()
    clip = clean.copy()
    for t in frames:
        clip[t][mask[t] == 1] += POP
    return clip, mask


def check_planes(images, mask, out, support, replaced):
    """Outside the mask: the input's bits and -1 in both planes; under it support counts and replaced is 0 or 1."""
    check_outside(images, mask, out, support)
    under = np.broadcast_to(mask == 1, replaced.shape)
    assert (replaced[~under] == -1).all() and np.isin(replaced[under], (0, 1)).all(), "replaced: -1 outside the mask, 0 or 1 under it"
    assert (support[replaced == 1] >= rref.QUORUM).all(), "(support[replaced == 1] >= rref.QUORUM).all()"


def check_pan_equals_plain(robust, plain):
    _, clip, mask = smooth_pan_clip()
    out, support, replaced = robust
    check_planes(clip, mask, out, support, replaced)
    assert (_f32_bits(out) == _f32_bits(plain[0])).all() and (support == plain[1]).all(), (
        "the robust smooth against the plain smooth: output bits and support")
    assert (replaced[mask == 1] == 0).all(), "nothing replaced under the mask"                  # nothing is rejected under either reference


def check_pop(robust, plain):
    clean, _, mask = smooth_pan_clip()
    clip, _ = pop_clip((3,))
    out, support, replaced = robust
    check_planes(clip, mask, out, support, replaced)
    assert (_f32_bits(out) == _f32_bits(clean)).all(), "out against the clean clip"                         # the clean clip, in every frame
    assert int((replaced == 1).sum()) == 224 and (replaced[3][mask[3] == 1] == 1).all(), (
        "224 replaced pixels, all of frame 3 under the mask among them")
    assert (_f32_bits(plain[0]) == _f32_bits(clip)).all(), "the plain smooth against the clip"                # the plain rule keeps the pop


def check_two_frame_pop(radius, robust):
    clean, _, mask = smooth_pan_clip()
    clip, _ = pop_clip((3, 4))
    out, support, replaced = robust
    check_planes(clip, mask, out, support, replaced)
    if radius == 1:                                                    # what lasts longer than R frames stays
        assert (_f32_bits(out) == _f32_bits(clip)).all() and not (replaced == 1).any(), "out against the clip"
    else:
        assert (_f32_bits(out) == _f32_bits(clean)).all() and int((replaced == 1).sum()) == 448, "out against the clean clip"
        assert (replaced[3:5][mask[3:5] == 1] == 1).all(), "(replaced[3:5][mask[3:5] == 1] == 1).all()"


def check_ghost_removed(robust):
    clip, mask = ghost_clip()
    still, _ = smooth_still_clip()
    out, support, replaced = robust
    check_planes(clip, mask, out, support, replaced)
    assert (_f32_bits(out) == _f32_bits(still)).all() and int((replaced == 1).sum()) == 48, (
        "out against the still clip bit for bit, 48 pixels replaced")


def check_robust_noise(radius, out, support, replaced):
    still, clip, mask = noise_clip()
    check_planes(clip, mask, out, support, replaced)
    assert not (replaced == 1).any(), "not (replaced == 1).any()"
    inner = slice(radius, clip.shape[0] - radius)
    before, after = (clip - still)[inner][:, mask == 1], (out - still)[inner][:, mask == 1]
    ratio = float(after.astype(np.float64).var() / before.astype(np.float64).var())
    print(f"radius {radius}: variance ratio {ratio:.4f}, the weights give {NOISE_RATIO[radius]:.4f}")
    assert abs(ratio / NOISE_RATIO[radius] - 1) <= 0.15, (radius, ratio)
