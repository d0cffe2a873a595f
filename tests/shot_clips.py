"""The clips of the shot detect tests, in plain numpy: low-pass canvases of different tone that pan by 2 pixels a frame under a
little noise, joined by hard cuts, and the three things that must not be called a cut -- a flash frame, a large box that moves
further than the search, and a plain pan.  White-noise canvases (tests/temporal_clips.py) are no use here: at pyramid level 2
two of them are the same grey mush.  Every clip is (images fp32 [F, H, W, 3], the frames at which a new shot begins).  At the end, the scores and the per-shot fill
case that tests/test_shots_host.py and tests/test_gpu_shots.py both use."""
import functools

import numpy as np

from tests import shots_ref as sref
from tests import temporal_fill_ref as tref

H, W = 96, 128
PAN = 2                                # pixels a frame, along x
NOISE = 0.01
TONES = {"dark": (0.05, 0.60), "bright": (0.40, 0.95), "mid": (0.20, 0.80)}    # they overlap: a cut moves most pixels, not all


def _low_pass(a, radius, passes=2):
    k = np.ones(2 * radius + 1) / (2 * radius + 1)
    for _ in range(passes):
        for axis in (0, 1):
            pad = [(radius, radius) if ax == axis else (0, 0) for ax in range(a.ndim)]
            a = np.apply_along_axis(lambda v: np.convolve(v, k, mode="valid"), axis, np.pad(a, pad, mode="wrap"))
    return a


@functools.lru_cache(maxsize=None)
def canvas(seed, tone, height=H, width=W + 64):
    """fp32 [height, width, 3]: low-frequency structure that fills the tone's range."""
    rng = np.random.default_rng([seed, 77])
    lo, hi = TONES[tone]
    c = _low_pass(rng.random((height, width, 3)), 4)
    c = (c - c.min((0, 1))) / (c.max((0, 1)) - c.min((0, 1)))
    return (lo + (hi - lo) * c).astype(np.float32)


def pan(frames, seed, tone, start=0):
    """`frames` frames cut out of one canvas, 2 pixels further along x each."""
    c = canvas(seed, tone)
    return np.stack([c[:, start + PAN * t:start + PAN * t + W] for t in range(frames)])


def _noisy(images, seed):
    rng = np.random.default_rng([seed, 78])
    return (images + rng.normal(0, NOISE, images.shape)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def one_shot(frames=10):
    return _noisy(pan(frames, 1, "mid"), 1), ()


@functools.lru_cache(maxsize=None)
def two_shots(frames=12, k=5):
    return _noisy(np.concatenate([pan(k, 2, "dark"), pan(frames - k, 3, "bright")]), 2), (k,)


@functools.lru_cache(maxsize=None)
def three_shots():
    return _noisy(np.concatenate([pan(5, 4, "bright"), pan(6, 5, "dark"), pan(5, 6, "mid")]), 3), (5, 11)


@functools.lru_cache(maxsize=None)
def close_cuts():
    """Two cuts two frames apart: closer than the default window."""
    return _noisy(np.concatenate([pan(6, 7, "dark"), pan(2, 8, "bright"), pan(6, 9, "dark")]), 4), (6, 8)


FLASH_AT = 5                           # the flash frame: the pairs FLASH_AT - 1 and FLASH_AT are high


@functools.lru_cache(maxsize=None)
def flash(frames=10, at=FLASH_AT):
    images = pan(frames, 10, "dark").copy()
    images[at] = np.clip(images[at] + 0.5, 0, 1)
    return _noisy(images, 5), ()


@functools.lru_cache(maxsize=None)
def fast_box(frames=10, step=17):
    """A bright 40 x 28 box on a dark pan that moves 17 pixels a frame: further than any search reaches at any level used."""
    images = pan(frames, 11, "dark").copy()
    box = canvas(12, "bright")[:40, :28]
    for t in range(frames):
        x = (5 + step * t) % (W - 28)
        images[t, 30:70, x:x + 28] = box
    return _noisy(images, 6), ()


CLIPS = {"one_shot": one_shot, "two_shots": two_shots, "three_shots": three_shots, "close_cuts": close_cuts, "flash": flash,
         "fast_box": fast_box}


def box_mask(frames, at, height=H, width=W):
    """fp32 [frames, height, width]: a box under the mask in the two frames beside the cut at `at`, nothing elsewhere."""
    mask = np.zeros((frames, height, width), np.float32)
    mask[at - 1:at + 1, height // 3:height // 3 + 20, width // 3:width // 3 + 24] = 1.0
    return mask


@functools.lru_cache(maxsize=None)
def scores(name, level=2, search=2):
    images, starts = CLIPS[name]()
    return (*sref.shot_scores(images, level, search), starts)


def expected_shot(frames, starts):
    return np.searchsorted(np.asarray(starts, dtype=np.int64), np.arange(frames), side="right").astype(np.int32)


FILL_FRAMES, FILL_CUT, FILL_LEVELS = 6, 3, 3


@functools.lru_cache(maxsize=None)
def fill_case():
    """(images, mask, ranges, the whole clip's fill, the per-shot composition): the two-shot clip, a box under the mask in the two
    frames beside the cut.  tests/test_gpu_shots.py compares the device with both."""
    images, starts = two_shots(FILL_FRAMES, FILL_CUT)
    mask = box_mask(FILL_FRAMES, FILL_CUT)
    ranges = [(0, FILL_CUT), (FILL_CUT, FILL_FRAMES)]
    whole = tref.temporal_fill_ref(images, mask, levels=FILL_LEVELS)
    parts = [tref.temporal_fill_ref(images[lo:hi], mask[lo:hi], levels=FILL_LEVELS) for lo, hi in ranges]
    source = np.concatenate([np.where(p[2] >= 0, p[2] + lo, p[2]) for p, (lo, hi) in zip(parts, ranges)])
    composed = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), source)
    return images, mask, ranges, whole, composed


def foreign_sources(source, mask, ranges):
    """The masked pixels whose source frame lies in another shot than the pixel."""
    shot = expected_shot(source.shape[0], [lo for lo, _ in ranges[1:]])
    of_source = shot[np.clip(source, 0, None)]
    return int(((mask >= 0.5) & (source >= 0) & (of_source != shot[:, None, None])).sum())
