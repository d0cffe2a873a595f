"""Clips of tens of frames for the temporal fill, the checked fill and the temporal smooth: plain numpy, no device.  The short
clips of the other test modules end before an origin is older than 4 frames, a smooth chain longer than 4 steps or a call has more
than 32 steps; these are built so that all of that happens, and tests/test_temporal_long_clips_host.py asserts that it does."""
import functools

import numpy as np

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
