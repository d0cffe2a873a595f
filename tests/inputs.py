"""Inputs the motion tests share: seeded generators, plane lists, the video and mask tables and the batch-job builders.
numpy only, no device."""
import functools

import numpy as np

from tests import propagate_anchored_ref as aref
from tests import propagate_anchored_visible_ref as avref
from tests import propagate_keys_visible_ref as kvref
from tests import propagate_ref as ref
from tests import stabilize_ref as stab
from tests.anchor_clips import subpixel_clip


# (23, 33) and (40, 70): odd at every pyramid level, no multiple of the 8-pixel block, the 16-pixel window or the 32-pixel tile;
# (40, 70) takes several workgroups of every kernel.  Levels 1 has no parent field; with 6 the top levels of (23, 33) are 1 x 2.
# "chunked": fp16 images and every WS_CAP_BYTES lowered, the restatement on the half-rounded values.
SMALL, LARGE = (23, 33), (40, 70)

# one under, at and one over the block (8) and the window (16), odd sizes at every pyramid level; (70, 130): several workgroups of
# every kernel (32 x 32 tiles, a 9 x 17 grid)
PLANES = [(1, 1), (1, 7), (7, 1), (8, 8), (9, 15), (16, 17), (23, 33), (40, 70)]

BIG = (70, 130)


def _rng(*key):
    return np.random.default_rng([abs(int(k)) for k in key])


def _video(F, H, W, C=3, seed=0):
    """Frames cut out of one random canvas, moving by (2, -3) pixels per frame, with a little noise of their own."""
    rng = _rng(F, H, W, C, seed)
    canvas = rng.random((H + 2 * F, W + 3 * F, C), dtype=np.float32)
    frames = [canvas[2 * t:2 * t + H, 3 * (F - 1 - t):3 * (F - 1 - t) + W] for t in range(F)]
    return (np.stack(frames) + rng.normal(0, 0.02, (F, H, W, C))).astype(np.float32)


def _constant(F, H, W, C=3, seed=0):
    return np.full((F, H, W, C), 0.375, np.float32)


def _wild_video(F, H, W, C=3, seed=0):
    """Values outside [0, 1], NaN and infinities."""
    rng = _rng(F, H, W, C, seed, 1)
    v = (3.0 * rng.random((F, H, W, C)) - 1.0).astype(np.float32)
    pick = rng.random((F, H, W, C))
    v[pick < 0.1] = np.nan
    v[(pick >= 0.1) & (pick < 0.15)] = np.inf
    v[(pick >= 0.15) & (pick < 0.2)] = -np.inf
    return v


VIDEOS = {"random": _video, "constant": _constant, "wild": _wild_video}


def _disc(H, W, seed=0):
    """A disc that touches the border."""
    yy, xx = np.mgrid[:H, :W]
    r = max(min(H, W) / 3, 1)
    return ((yy - r + 1) ** 2 + (xx - W + r) ** 2 <= r * r).astype(np.float32)


def _soft(H, W, seed=0):
    return _rng(H, W, seed, 2).random((H, W), dtype=np.float32)


def _threshold(H, W, seed=0):
    v = np.float32(0.5)
    return _rng(H, W, seed, 3).choice(np.array([np.nextafter(v, np.float32(0)), v, np.nextafter(v, np.float32(1))]), (H, W))


def _wild_mask(H, W, seed=0):
    rng = _rng(H, W, seed, 4)
    m = (3.0 * rng.random((H, W)) - 1.0).astype(np.float32)
    pick = rng.random((H, W))
    m[pick < 0.15] = np.nan
    m[(pick >= 0.15) & (pick < 0.2)] = np.inf
    m[(pick >= 0.2) & (pick < 0.25)] = -np.inf
    return m


def _pixels(H, W, n):
    """n mask pixels in the top left corner, all inside block (0, 0)'s window."""
    m = np.zeros((H, W), np.float32)
    m.reshape(-1)[[y * W + x for y in range(min(H, 4)) for x in range(min(W, 4))][:n]] = 1
    return m


MASKS = {"empty": lambda H, W, s=0: np.zeros((H, W), np.float32), "full": lambda H, W, s=0: np.ones((H, W), np.float32),
         "one pixel": lambda H, W, s=0: _pixels(H, W, 1), "15 pixels": lambda H, W, s=0: _pixels(H, W, 15),
         "16 pixels": lambda H, W, s=0: _pixels(H, W, 16), "disc": _disc, "soft": _soft, "threshold": _threshold, "wild": _wild_mask}


@functools.lru_cache(maxsize=None)
def _advance_case(H, W, scale):
    rng = _rng(H, W, scale)
    gh, gw = ref.grid_of(H, W)
    vec = rng.integers(-scale, scale + 1, (gh, gw, 2)).astype(np.int32)
    vec2 = rng.integers(-scale, scale + 1, (gh, gw, 2)).astype(np.int32)
    bits = (rng.random((H, W)) < 0.5).astype(np.uint8)
    P1, c1 = ref.advance(ref.key_positions(H, W), vec, bits)
    P2, c2 = ref.advance(P1, vec2, bits)
    return vec, vec2, bits, P1, c1, P2, c2


def _anchored_lumas(kind, H, W):
    """(Yt, Yk) uint8.  noisy: a random key plane and the same plane moved by (1, -1) plus noise, so the winner is mostly off the
    centre and the sub-pixel step has work; flat: two values only, so candidates tie and the key order decides."""
    rng = _rng(H, W, 19)
    if kind == "noisy":
        Yk = rng.integers(0, 256, (H, W))
        Yt = np.roll(Yk, (1, -1), (0, 1)) + np.round(rng.normal(0, 12, (H, W)))
    else:
        Yk = 128 + rng.integers(0, 2, (H, W))
        Yt = 128 + rng.integers(0, 2, (H, W))
    return np.clip(Yt, 0, 255).astype(np.uint8), Yk.astype(np.uint8)


def _border_disc(H, W):
    """A disc that touches the border."""
    yy, xx = np.mgrid[:H, :W]
    r = max(min(H, W) / 3, 1)
    return ((yy - r + 1) ** 2 + (xx - W + r) ** 2 <= r * r).astype(np.uint8)


def _random(H, W):
    """The density grows from 0.02 on the left to 0.5 on the right: windows under LP_PROP_MIN_PIXELS, at it and over it."""
    density = 0.02 + 0.48 * np.arange(W)[None, :] / max(W - 1, 1)
    return (_rng(H, W, 20).random((H, W)) < density).astype(np.uint8)


ANCHORED_MASKS = {"empty": lambda H, W: np.zeros((H, W), np.uint8), "full": lambda H, W: np.ones((H, W), np.uint8), "disc": _border_disc,
                  "random": _random}


def _positions(kind, H, W):
    """int64 [H, W, 2] in 1/16 px: the key map; the key map bent by a smooth field plus jitter; a map that leaves the plane."""
    P = ref.key_positions(H, W)
    if kind == "key":
        return P
    yy, xx = np.mgrid[:H, :W]
    if kind == "smooth":
        bend = np.stack([40 * np.sin(xx / 9.0) + 25 * np.cos(yy / 5.0), 55 * np.cos(xx / 7.0 + yy / 11.0)], axis=-1)
        return P + np.round(bend).astype(np.int64) + _rng(H, W, 7).integers(-8, 9, (H, W, 2))
    return (3 * P) // 2 - 16 * 5 + _rng(H, W, 8).integers(-300, 301, (H, W, 2))


def _anchored_inputs(plane, positions, lumas, mask):
    H, W = plane
    return _positions(positions, H, W), *_anchored_lumas(lumas, H, W), ANCHORED_MASKS[mask](H, W)


def _visible_lumas(kind, H, W):
    """(Yt, Yk) uint8.  noisy: the key's plane plus noise whose amplitude grows from 0 to 60 grey levels from left to right, so the
    residual crosses every threshold somewhere; dark: t darker than the key by 20 on the left to 60 on the right, so D is strongly
    negative, the floor of a negative mean is taken and mu runs into its clamp at -32."""
    rng = _rng(H, W, 9)
    xx = np.broadcast_to(np.arange(W)[None, :] / max(W - 1, 1), (H, W))
    if kind == "noisy":
        Yk = rng.integers(0, 256, (H, W))
        Yt = Yk + np.round(rng.normal(0, 1, (H, W)) * 60 * xx)
    else:
        Yk = 190 + rng.integers(0, 60, (H, W))
        Yt = Yk - np.round(20 + 40 * xx) - rng.integers(0, 3, (H, W))
    return np.clip(Yt, 0, 255).astype(np.uint8), Yk.astype(np.uint8)


def _anchored_visible_lumas(kind, H, W):
    """(Yt, Yk) uint8.  noisy: a random key plane and the same plane moved by (1, -1) plus noise whose amplitude grows from 0 to 60
    grey levels from left to right, so the winner is mostly off the centre and the gate's residual crosses every threshold
    somewhere; dark: the visible test's kind, t darker than the key by 20 to 60, so mu runs into its clamp at -32."""
    if kind == "dark":
        return _visible_lumas("dark", H, W)
    rng = _rng(H, W, 21)
    xx = np.broadcast_to(np.arange(W)[None, :] / max(W - 1, 1), (H, W))
    Yk = rng.integers(0, 256, (H, W))
    Yt = np.roll(Yk, (1, -1), (0, 1)) + np.round(rng.normal(0, 1, (H, W)) * 60 * xx)
    return np.clip(Yt, 0, 255).astype(np.uint8), Yk.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _anchored_visible_inputs(plane, positions, lumas, mask):
    """(P, Yt, Yk, m) in numpy, shared: not to be written to."""
    H, W = plane
    return _positions(positions, H, W), *_anchored_visible_lumas(lumas, H, W), ANCHORED_MASKS[mask](H, W)


ANCHORED_VISIBLE_LEVELS = 3


@functools.lru_cache(maxsize=None)
def _anchored_visible_clip(F, H, W, key, seed=0):
    """The sub-pixel clip with something in front of the subject on every frame but the key: three columns of another texture
    through the disc's right half, so that blocks are gated and flags fire from the first step on."""
    images, truth = subpixel_clip(F, H, W, seed=seed)
    x = int(0.3 * W + min(H, W) / 10)
    bar = _rng(H, W, 22).random((H, 3, 1)).astype(np.float32)
    for f in range(F):
        if f != key:
            images[f, :, x:x + 3, :] = bar
    images.setflags(write=False)
    return images, truth


@functools.lru_cache(maxsize=None)
def _anchored_visible_want(F, H, W, key):
    images, truth = _anchored_visible_clip(F, H, W, key)
    trace = {}
    want = avref.propagate_anchored_visible_ref(images, truth[key].astype(np.float32), key, ANCHORED_VISIBLE_LEVELS, 2, 8, 2, 16, trace)
    return want, trace


KEYS_PARAMS = [(1, 1, 0), (3, 2, 8), (6, 7, 64)]                           # levels, search, smooth
KEYS_JOB_MASKS = ("disc", "soft", "full", "16 pixels", "wild", "threshold", "empty")
KEYS_SPECIAL = [1, -1, 2, -2, 3, -3, 4095, 4096, 4097, -4095, -4096, -4097, stab.Q_FAR, -stab.Q_FAR, 2 * 16383 ** 2, -2 * 16383 ** 2]
KEYS_ANCHORED_LEVELS, KEYS_ANCHORED_SEARCH, KEYS_ANCHORED_SMOOTH, KEYS_ANCHORED_ANCHOR = 3, 2, 8, 2

# (1, 1), (7, 9), (33, 70): no side a multiple of 4 or 32, the scalar path; (40, 72): the vector path, several tiles
BATCH_PLANES = [(1, 1), (7, 9), (33, 70), (40, 72)]

JOB_POSITIONS = ("key", "smooth", "outside")
JOB_MASKS = ("disc", "random", "15 pixels", "full", "empty")              # job 2 of a launch has 15 pixels: under LP_PROP_MIN_PIXELS


def _random_mask(H, W, i):
    density = 0.02 + 0.48 * np.arange(W)[None, :] / max(W - 1, 1)
    return (_rng(H, W, i, 21).random((H, W)) < density).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _job(H, W, i):
    """Job i of a plane, the same in every launch that holds it: (P int32 [H, W, 2], Yt, Yk, m uint8 [H, W]).  The frame is the key
    moved by (1, -1) plus noise, so the winner is mostly off the centre and the sub-pixel step has work."""
    rng = _rng(H, W, i, 38)
    Yk = rng.integers(0, 256, (H, W))
    Yt = np.clip(np.roll(Yk, (1, -1), (0, 1)) + np.round(rng.normal(0, 12, (H, W))), 0, 255)
    P = _positions(JOB_POSITIONS[i % 3], H, W) + (0 if i % 3 == 0 else rng.integers(-6, 7, (H, W, 2)))
    kind = JOB_MASKS[i % len(JOB_MASKS)]
    m = _random_mask(H, W, i) if kind == "random" else MASKS[kind](H, W, i)
    out = (P.astype(np.int32), Yt.astype(np.uint8), Yk.astype(np.uint8), ref.binarise(m).astype(np.uint8))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _job_field(H, W, i, anchor, smooth):
    P, Yt, Yk, m = _job(H, W, i)
    return aref.anchor_field(P.astype(np.int64), Yt, Yk, m, anchor, smooth)


# per plane: the frames, then one key first, in the middle, last; two adjacent keys (no in-between frame); both ends; three keys
KEYS_ANCHORED_CLIPS = {(9, 7): (6, [[0], [3], [5], [2, 3], [0, 5], [0, 2, 5]]), (40, 70): (7, [[0], [3], [6], [2, 3], [0, 6], [0, 3, 6]])}


@functools.lru_cache(maxsize=None)
def _keys_anchored_clip(plane, half=False):
    """(images, their luma planes, their luma pyramids, a painting per frame).  (40, 70): the disc that moves a fraction of a pixel
    a frame, painted with the truth; (9, 7), too small for it: the moving canvas under random paintings."""
    F = KEYS_ANCHORED_CLIPS[plane][0]
    if plane == (9, 7):
        images, painted = _video(F, *plane, 3, seed=38), np.stack([_soft(*plane, k) for k in range(F)])
    else:
        images, truth = subpixel_clip(F, *plane, vy=0.43, vx=0.71)
        painted = truth.astype(np.float32)
    if half:
        images = images.astype(np.float16).astype(np.float32)
    Y = ref.luma(images)
    for a in (images, painted):
        a.setflags(write=False)
    return images, Y, [ref.pyramid(Y[f], KEYS_ANCHORED_LEVELS, ref.down_luma) for f in range(F)], painted


VISIBLE_MASKS = {"empty": lambda H, W: np.zeros((H, W), np.uint8), "full": lambda H, W: np.ones((H, W), np.uint8), "disc": _border_disc,
         # about 14 mask pixels per 16 x 16 window: some windows under LP_PROP_MIN_PIXELS, some at it, some over
         "sparse": lambda H, W: (_rng(H, W, 10).random((H, W)) < 0.055).astype(np.uint8)}


def _visible_job(H, W, job):
    """Inputs of one job, different for every job: the positions' and the lumas' kinds and the mask's form cycle, and the planes
    are rolled by the job's number."""
    P = np.roll(_positions(("key", "smooth", "outside")[job % 3], H, W), job, axis=1)
    Yt, Yk = _visible_lumas(("noisy", "dark")[job % 2], H, W)
    m = list(VISIBLE_MASKS.values())[(job + 1) % len(VISIBLE_MASKS)](H, W)
    return P, np.roll(Yt, job, axis=0), Yk, np.roll(m, -job, axis=1)


def _flags(kind, gh, gw):
    yy, xx = np.mgrid[:gh, :gw]
    return {"none": np.zeros((gh, gw), np.int64), "all": np.ones((gh, gw), np.int64), "checkerboard": (yy + xx) % 2,
            "random": _rng(gh, gw, 11).integers(0, 2, (gh, gw))}[kind]


def _occlude_job(H, W, job):
    flags = np.roll(_flags(("random", "checkerboard", "none", "all")[job % 4], *ref.grid_of(H, W)), job, axis=1)
    c = _rng(H, W, 12, job).integers(0, 257, (H, W))
    c[_rng(H, W, 13, job).random((H, W)) < 0.3] = 256
    return c, flags


def _counts(kind, span):
    """(N_A, N_B) by step.  The forward chain is at step j on frame j of the gap, the backward chain at step span - j."""
    a, b = [200] * span, [300] * span
    mid = (span + 1) // 2
    if kind == "a_lost":
        a[mid] = 15                                                    # lost from the middle frame on, sticky: later counts are high again
    if kind == "b_lost":
        b[mid] = 0                                                     # lost from its step `mid` on: the frames up to span - mid
    if kind == "both_lost":                                            # either from its first step on: both on every frame
        a[1], b[1] = 15, 0
    if kind == "small_key":                                            # a key below 16 bits is never lost, whatever follows
        a = [15] + [0] * (span - 1)
        b = [16] + [16] * (span - 1)
    return a, b


def _merge_want(q, c, cv, f, na, nb, span):
    out = [kvref.merge_frame(q[0, i], q[1, i], (c[0, i], cv[0, i], f[0, i]), (c[1, i], cv[1, i], f[1, i]), kvref.lost_at(na, i + 1),
                             kvref.lost_at(nb, span - i - 1), span, i + 1) for i in range(span - 1)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


# one under, at and over the block (8) and the window (16), and several workgroups (32 x 32 tiles); the last two have a width that
# is a multiple of 4, where the kernels read and write four pixels as one vector
VISIBLE_PLANES = [(1, 1), (1, 7), (7, 1), (8, 8), (9, 15), (16, 17), (23, 33), (40, 70), (70, 130), (33, 64), (70, 132)]


@functools.lru_cache(maxsize=None)
def _occluded_video(F, H, W):
    """Frames cut out of one random canvas, moving by (2, -3) pixels per frame, a little noise of their own, and a static bar of
    another texture over the middle fifth of the width: (images fp32 [F, H, W, 3], a centred disc as the key mask)."""
    rng = _rng(F, H, W, 14)
    canvas = rng.random((H + 2 * F, W + 3 * F, 3), dtype=np.float32)
    frames = np.stack([canvas[2 * t:2 * t + H, 3 * (F - 1 - t):3 * (F - 1 - t) + W] for t in range(F)])
    frames = frames + rng.normal(0, 0.02, frames.shape)
    x0, x1 = 2 * W // 5, 3 * W // 5
    frames[:, :, x0:x1] = rng.random((H, x1 - x0, 3), dtype=np.float32)
    yy, xx = np.mgrid[:H, :W]
    mask = ((yy - H / 2) ** 2 + (xx - W / 2) ** 2 <= (min(H, W) / 2.5) ** 2).astype(np.float32)
    return frames.astype(np.float32), mask


def _random_scores(frames, n, seed):
    """Heavy-tailed residuals with runs of equal values, so that some pair stands out of every window and equal neighbours occur."""
    rng = _rng(frames, seed, 9)
    A = rng.integers(1, 255, frames - 1) ** 2 * n // 256
    B = rng.integers(0, 2 * n + 1, frames - 1)
    run = rng.random(frames - 1) < 0.3
    for t in range(1, frames - 1):
        if run[t]:
            A[t] = A[t - 1]
    return np.stack([A, B], axis=1).astype(np.int64)


FILL_FRAMES, FILL_LEVELS = 5, 3
ALL_PLANES = PLANES + [BIG]
plane_ids = lambda s: "x".join(map(str, s))                          # noqa: E731


def _random_masks(frames, H, W, seed=0, share=0.3):
    return (_rng(frames, H, W, seed, 5).random((frames, H, W)) < share).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _carry_case(H, W, wild, channels=3):
    """A frame 2 of 5 with random known bits, a random field of up to 2.5 pixels, a random state of both neighbours with origins
    in every frame, and a random `source` under the mask from an earlier pass."""
    rng = _rng(H, W, int(wild), 6)
    images = (_wild_video if wild else _video)(FILL_FRAMES, H, W, channels)
    gh, gw = ref.grid_of(H, W)
    vec = rng.integers(-40, 41, (gh, gw, 2)).astype(np.int32)
    known = (rng.random((3, H, W)) < 0.5).astype(np.uint8)            # of the frames 1, 2, 3
    org = rng.integers(-1, FILL_FRAMES, (H, W)).astype(np.int32)
    pos = np.stack([rng.integers(-40, 16 * H + 40, (H, W)), rng.integers(-40, 16 * W + 40, (H, W))], axis=-1).astype(np.int32)
    source = np.where(known[1] != 0, 2, rng.choice([-1, 0, 1, 3, 4], (H, W))).astype(np.int32)
    return images, vec, known, org, pos, source


# One block high with several across, and the other way round: the grid is one block wide, so both blocks a pixel interpolates
# between are the same clamped one.  The plane list's own thin planes (1 x 1, 1 x 7, 7 x 1) are thinner than the case's vectors are
# long: there every masked pixel's vector leaves the plane and its value is never seen (counted on the restatement alone).
THIN_PLANES = [(7, 33), (33, 5)]
