"""Scenes of the mask-propagate tests and the quality lines that a host test and its device twin both check.
numpy and the restatements only, no device."""
import functools

import numpy as np

from tests import propagate_anchored_ref as aref
from tests import propagate_anchored_visible_ref as avref
from tests import propagate_keys_anchored_ref as karef
from tests import propagate_keys_anchored_visible_ref as kavref
from tests import propagate_keys_ref as kref
from tests import propagate_keys_visible_ref as kvref
from tests import propagate_ref as ref
from tests import propagate_visible_ref as vref
from tests.anchor_clips import _tex, iou, subpixel_clip


@functools.lru_cache(maxsize=None)
def drift_case():
    """subpixel_clip(33, 40, 56), the key on frame 0: (images, truth, the plain restatement's output, the anchored one's with the
    defaults).  Shared with the GPU test, which compares the device's output with the last."""
    images, truth = subpixel_clip(33, 40, 56)
    key = truth[0].astype(np.float32)
    return images, truth, ref.propagate_ref(images, key, 0, 4, 2, 8), aref.propagate_anchored_ref(images, key, 0, 4, 2, 8, 2)


def assert_the_two_drift_iou_lines(truth, plain, anchored):
    """The proof that the rule does what it is for.  Measured on the restatement: 0.484 and a minimum of 0.868; the margins cover
    nothing but a reader's rewording of the restatement."""
    last = iou(plain[-1] >= 0.5, truth[-1])
    worst = min(iou(anchored[t] >= 0.5, truth[t]) for t in range(len(truth)))
    print("plain, last frame", last, "anchored, worst frame", worst)
    assert last < 0.65, "last < 0.65"
    assert worst >= 0.80, "worst >= 0.80"


QUALITY_DEFAULTS = (0, 4, 2, 8)                                                 # key_frame, levels, search, smooth
QUALITY_ANCHOR, QUALITY_OCCLUSION = 2, 16


def occluded_clip(name):
    """Clip A: subpixel_clip(33, 64, 96) with a static textured bar on columns 50..55 of every frame, at most 28 % of the subject
    behind it on any frame.  Clip B: the same with rows 20..25, so the bar crosses the subject on every frame, the key frame
    included.  (images, truth, bar bool [H, W])."""
    images, truth = subpixel_clip(33, 64, 96)
    bar = np.zeros((64, 96), bool)
    if name == "A":
        images[:, :, 50:56, :] = _tex(np.random.default_rng(99), 64, 6)[None, :, :, None]
        bar[:, 50:56] = True
    else:
        images[:, 20:26, :, :] = _tex(np.random.default_rng(99), 6, 96)[None, :, :, None]
        bar[20:26] = True
    return images, truth, bar


@functools.lru_cache(maxsize=None)
def anchored_quality_case(name):
    """(images, truth, the new restatement's (mask, hidden), the anchored restatement's mask, the visible one's (mask, hidden)) at
    the defaults, the key truth[0] on frame 0.  "N": subpixel_clip(33, 40, 56), no occluder.  Shared with the GPU test, which
    compares the device's output with the first."""
    images, truth = subpixel_clip(33, 40, 56) if name == "N" else occluded_clip(name)[:2]
    key = truth[0].astype(np.float32)
    return (images, truth, avref.propagate_anchored_visible_ref(images, key, *QUALITY_DEFAULTS, QUALITY_ANCHOR, QUALITY_OCCLUSION),
            aref.propagate_anchored_ref(images, key, *QUALITY_DEFAULTS, QUALITY_ANCHOR),
            vref.propagate_visible_ref(images, key, *QUALITY_DEFAULTS, QUALITY_OCCLUSION))


def whole_subject_iou(mask, hidden, truth):
    """(last frame, worst frame behind the key) of iou((mask + hidden)[t] >= 0.5, truth[t])."""
    v = [iou((mask[t] + hidden[t]) >= 0.5, truth[t]) for t in range(1, len(truth))]
    return v[-1], min(v)


# the anchored and the visible form's last-frame whole-subject IoU may be at most this
QUALITY_LINES = {"A": (0.70, 0.30), "B": (0.50, 0.50)}


def assert_the_anchored_quality_lines(name, truth, new, anchored, visible):
    """The proof that the rule does what it is for: whole-subject IoU, hidden = 0 for the anchored form.  Measured on the
    restatements, last frame / worst frame:
        A: new 0.917 / 0.914, anchored 0.621 / 0.621, visible 0.142 / 0.142   (without the gate 0.720 / 0.720)
        B: new 0.964 / 0.914, anchored 0.386 / 0.381, visible 0.067 / 0.067   (without the gate 0.361 / 0.361)
    The margins cover a reader's rewording of the restatement and nothing else.  IoU of `mask` alone against the visible part of
    the subject on A: 0.604 on the last and on the worst frame (the block-wide flags hide up to a block beyond the bar); recorded,
    nothing is asserted on it."""
    new_last, new_worst = whole_subject_iou(*new, truth)
    anchored_last, _ = whole_subject_iou(anchored, np.zeros_like(anchored), truth)
    visible_last, _ = whole_subject_iou(*visible, truth)
    print(name, "new, last and worst frame", new_last, new_worst, "anchored, last frame", anchored_last, "visible, last frame", visible_last)
    assert new_worst >= 0.85, "new_worst >= 0.85"
    assert anchored_last <= QUALITY_LINES[name][0], "anchored_last <= QUALITY_LINES[name][0]"
    assert visible_last <= QUALITY_LINES[name][1], "visible_last <= QUALITY_LINES[name][1]"


@functools.lru_cache(maxsize=None)
def texture(seed, H=256, W=256, beta=1.2):
    """A periodic random texture with a 1 / f^beta amplitude spectrum, scaled to [0, 1]."""
    rng = np.random.default_rng(seed)
    fy, fx = np.fft.fftfreq(H)[:, None], np.fft.fftfreq(W)[None, :]
    f = np.sqrt(fy * fy + fx * fx)
    f[0, 0] = 1.0
    spec = (rng.normal(size=(H, W)) + 1j * rng.normal(size=(H, W))) / f ** beta
    spec[0, 0] = 0
    t = np.fft.ifft2(spec).real
    return (t - t.min()) / (t.max() - t.min())


def _sample(tex, yy, xx):
    H, W = tex.shape
    y0, x0 = np.floor(yy).astype(int), np.floor(xx).astype(int)
    fy, fx = yy - y0, xx - x0
    g = lambda y, x: tex[y % H, x % W]                                # noqa: E731
    return (1 - fy) * ((1 - fx) * g(y0, x0) + fx * g(y0, x0 + 1)) + fy * ((1 - fx) * g(y0 + 1, x0) + fx * g(y0 + 1, x0 + 1))


def disc_scene(F, v_obj, v_bg, radius, centre, seed=0, H=96, W=128, sigma=0.01):
    """A disc carrying one texture moves by v_obj pixels per frame over a background texture that moves by v_bg, both sampled
    bilinearly, Gaussian noise on every frame: (images fp32 [F, H, W, 1], the true disc per frame)."""
    bg, ob = texture((seed, 1)), texture((seed, 2))
    rng = np.random.default_rng([seed, 3])
    yy, xx = np.mgrid[:H, :W].astype(np.float64)
    frames, discs = [], []
    for t in range(F):
        disc = (yy - centre[0] - v_obj[0] * t) ** 2 + (xx - centre[1] - v_obj[1] * t) ** 2 <= radius ** 2
        img = np.where(disc, _sample(ob, yy - v_obj[0] * t, xx - v_obj[1] * t), _sample(bg, yy - v_bg[0] * t, xx - v_bg[1] * t))
        frames.append(img + rng.normal(0, sigma, img.shape))
        discs.append(disc)
    return np.stack(frames).astype(np.float32)[..., None], np.stack(discs)


SCENES = {"slow": (10, (1.3, -0.7), (0.3, -0.4), 18, (40, 70)), "still background": (12, (0.4, 0.3), (0.0, 0.0), 18, (40, 60)),
          "fast": (8, (3.3, -2.6), (-0.5, 0.5), 14, (30, 85))}


@functools.lru_cache(maxsize=None)
def gap_drift_case():
    """subpixel_clip(49, 40, 72) with the true discs painted on frames 8 and 40, levels 3: (images, truth, the several-keys
    restatement's output, the anchored one's).  Shared with the GPU test, which compares the device's output with the last."""
    images, truth = subpixel_clip(49, 40, 72)
    masks = truth[[8, 40]].astype(np.float32)
    return (images, truth, kref.propagate_keys_ref(images, masks, [8, 40], 3, 2, 8),
            karef.propagate_keys_anchored_ref(images, masks, [8, 40], 3, 2, 8, 2))


def lowest_iou(out, truth):
    return min(iou(out[t] >= 0.5, truth[t]) for t in range(len(truth)))


def assert_the_two_gap_iou_lines(truth, plain, anchored):
    """What the form is for: half way through the gap the plain chains have both fallen behind, the anchored ones have not.
    The restatement gives 0.737 and 0.871; the bounds are the issue's."""
    low_plain, low_anchored = lowest_iou(plain, truth), lowest_iou(anchored, truth)
    print("several keys, lowest per-frame IoU", low_plain, "anchored", low_anchored)
    assert low_anchored >= 0.85, "low_anchored >= 0.85"
    assert low_plain <= 0.78, "low_plain <= 0.78"


def _texture(rng, H, W, beta=1.2):
    """A periodic random texture with a 1 / f^beta amplitude spectrum, scaled to [0, 1]."""
    fy, fx = np.fft.fftfreq(H)[:, None], np.fft.fftfreq(W)[None, :]
    f = np.sqrt(fy * fy + fx * fx)
    f[0, 0] = 1.0
    spec = (rng.normal(size=(H, W)) + 1j * rng.normal(size=(H, W))) / f ** beta
    spec[0, 0] = 0
    t = np.fft.ifft2(spec).real
    return (t - t.min()) / (t.max() - t.min())


def occluded_disc_clip(seed, F, H, W, radius, bar, speed=3, noise=0.01):
    """A static random-texture background; a disc with a texture of its own that moves `speed` pixels per frame from the left
    edge; a static bar over columns bar[0]..bar[1] - 1 with a third texture, drawn over everything; Gaussian noise per frame.
    (images fp32 [F, H, W, 1], the whole disc per frame bool [F, H, W], the bar bool [H, W])."""
    rng = np.random.default_rng(seed)
    bg, ob, bt = (_texture(rng, 128, 256) for _ in range(3))
    yy, xx = np.mgrid[:H, :W]
    on_bar = (xx >= bar[0]) & (xx < bar[1])
    frames, discs = [], []
    for t in range(F):
        disc = (yy - H // 2) ** 2 + (xx - (radius + 2 + speed * t)) ** 2 <= radius * radius
        img = np.where(disc, ob[yy, (xx - speed * t) % 256], bg[:H, :W])
        img = np.where(on_bar, bt[:H, :W], img)
        frames.append(img + rng.normal(0, noise, img.shape))
        discs.append(disc)
    return np.stack(frames).astype(np.float32)[..., None], np.stack(discs), on_bar


@functools.lru_cache(maxsize=None)
def keys_quality_case(name):
    """(images, masks, keys, levels, truth, the new restatement's (mask, hidden), its trace, the keys-visible restatement's
    (mask, hidden), the keys-anchored one's mask).  "A", "B": tests/test_propagate_anchored_visible_host.py's occluded clips with the
    truth painted on the first and the last frame, the defaults.  "disc": occluded_disc_clip(0, 16, 64, 96, 12, (28, 44)), keys 0 and
    15, levels 3.  Shared with the GPU test, which compares the device's outputs with the new restatement's."""
    if name == "disc":
        images, truth, _ = occluded_disc_clip(seed=0, F=16, H=64, W=96, radius=12, bar=(28, 44))
        levels = 3
    else:
        images, truth, _ = occluded_clip(name)
        levels = 4
    keys = [0, len(truth) - 1]
    masks = truth[keys].astype(np.float32)
    trace = {}
    new = kavref.propagate_keys_anchored_visible_ref(images, masks, keys, levels, 2, 8, 2, 16, trace=trace)
    return (images, masks, keys, levels, truth, new, trace, kvref.propagate_keys_visible_ref(images, masks, keys, levels, 2, 8, 16),
            karef.propagate_keys_anchored_ref(images, masks, keys, levels, 2, 8, 2))


def whole_subject(mask, hidden, truth, frames):
    """(worst, mean) over `frames` of iou((mask + hidden)[t] >= 0.5, truth[t])."""
    v = [iou((mask[t] + hidden[t]) >= 0.5, truth[t]) for t in frames]
    return min(v), sum(v) / len(v)


def assert_the_keys_quality_lines(name, truth, new, keys_visible, keys_anchored):
    """What the form is for, whole-subject IoU with hidden = 0 for the keys-anchored form.  Measured on the restatements:
        A, worst frame of all:      new 0.910, keys-visible 0.770, keys-anchored 0.781
        B, worst frame of all:      new 0.894, keys-visible 0.669, keys-anchored 0.807
        disc, mean / worst of 1..14: new 0.946 / 0.837, keys-visible 0.967 / 0.921, keys-anchored 0.243 / 0.000
    The bounds are the issue's; the rule is integer arithmetic, so the margins cover a rewording of the restatement only."""
    frames = range(1, len(truth) - 1) if name == "disc" else range(len(truth))
    worst, mean = whole_subject(*new, truth, frames)
    kv_worst, kv_mean = whole_subject(*keys_visible, truth, frames)
    ka_worst, ka_mean = whole_subject(keys_anchored, np.zeros_like(keys_anchored), truth, frames)
    print(name, "new worst / mean", worst, mean, "keys-visible", kv_worst, kv_mean, "keys-anchored", ka_worst, ka_mean)
    if name == "disc":
        assert mean >= 0.85, "mean >= 0.85"
        assert ka_mean <= 0.5, "ka_mean <= 0.5"
    else:
        assert worst >= 0.85, "worst >= 0.85"
        assert kv_worst <= {"A": 0.80, "B": 0.72}[name], "kv_worst <= {\"A\": 0.80, \"B\": 0.72}[name]"
        assert ka_worst <= 0.83, "ka_worst <= 0.83"
    return worst, mean, kv_worst, kv_mean, ka_worst, ka_mean


def _moving(F, H, W, seed=21):
    """Frames cut out of one canvas that moves by (1, -2) per frame, a little noise, and a static bar of another texture."""
    rng = np.random.default_rng(seed)
    canvas = rng.random((H + F, W + 2 * F, 3), dtype=np.float32)
    frames = np.stack([canvas[t:t + H, 2 * (F - 1 - t):2 * (F - 1 - t) + W] for t in range(F)]) + rng.normal(0, 0.02, (F, H, W, 3))
    frames[:, :, 2 * W // 5:3 * W // 5] = rng.random((H, 3 * W // 5 - 2 * W // 5, 3), dtype=np.float32)
    return frames.astype(np.float32)


def _moving_disc(H, W, cy, cx, r):
    yy, xx = np.mgrid[:H, :W]
    return ((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r).astype(np.float32)
