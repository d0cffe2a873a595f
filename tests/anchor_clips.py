"""The clip the anchored video mask propagate is measured on, plain numpy: a textured disc moves a fraction of a pixel per frame
over a still textured background, a little noise on every frame.  The plain chain composes one-frame fields whose sub-pixel part is
pulled towards zero, so its mask falls behind the disc; `truth` is the disc per frame."""
import numpy as np


def _tex(rng, h, w):
    a = rng.random((h, w))
    for ax in (0, 1):
        a = (np.roll(a, -1, ax) + 2 * a + np.roll(a, 1, ax)) / 4
    return (a - a.min()) / (a.max() - a.min())


def subpixel_clip(F, H, W, vy=0.23, vx=0.61, noise=0.01, seed=0):
    """(images fp32 [F, H, W, 3], truth bool [F, H, W])."""
    rng = np.random.default_rng([F, H, W, seed, 36])
    bg, subj = _tex(rng, H, W), _tex(rng, 2 * H, 2 * W)
    yy, xx = np.mgrid[:H, :W].astype(np.float64)
    R, cy0, cx0 = min(H, W) / 5, 0.35 * H, 0.3 * W
    frames, truth = [], []
    for t in range(F):
        inside = (yy - cy0 - vy * t) ** 2 + (xx - cx0 - vx * t) ** 2 <= R * R
        sy, sx = yy - vy * t + H / 2, xx - vx * t + W / 2
        iy, ix = np.floor(sy).astype(int), np.floor(sx).astype(int)
        fy, fx = sy - iy, sx - ix
        s = (1 - fy) * ((1 - fx) * subj[iy, ix] + fx * subj[iy, ix + 1]) + fy * ((1 - fx) * subj[iy + 1, ix] + fx * subj[iy + 1, ix + 1])
        f = np.where(inside, s, bg) + rng.normal(0, noise, (H, W))
        frames.append(np.repeat(f[..., None], 3, -1)); truth.append(inside)
    return np.stack(frames).astype(np.float32), np.stack(truth)


def iou(a, b):
    return float((a & b).sum()) / max(int((a | b).sum()), 1)
