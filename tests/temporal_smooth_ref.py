"""numpy restatement of the video temporal smooth rule, written from include/lanpaint_hip.h (lp_tsmooth): every masked pixel is pulled
towards the weighted mean of what the neighbouring frames hold at the same scene point, as far as that agrees with it.  The motion
is the temporal fill's step field (tests/temporal_fill_ref.py, tests/propagate_ref.py); a position in 1/16 pixel is stepped along
it into the past and into the future, and the picture is sampled there with the temporal fill's `sample`.  Nothing here looks at
the kernels."""
from math import comb

import numpy as np

from tests import propagate_ref as ref
from tests import temporal_fill_ref as tref

MOTIONS = ("background", "picture")


def weights(radius):
    """w_0 .. w_R = C(2R, R + k)."""
    return [comb(2 * radius, radius + k) for k in range(radius + 1)]


def fields(images, known, motion="background", levels=4, search=2, smooth=8):
    """(fwd, bwd): int64 [F, gh, gw, 2] each; fwd[u] is the field of frame u towards u + 1 (row F - 1 is zero and never used),
    bwd[u] towards u - 1 (row 0 likewise).  `known` uint8 [F, H, W]; with motion "picture" every pixel weighs in."""
    F, H, W = images.shape[:3]
    Y = ref.luma(images)
    pyr = [ref.pyramid(Y[f], levels, ref.down_luma) for f in range(F)]
    kpyr = tref.known_pyramids(known if motion == "background" else np.ones_like(known), levels)
    gh, gw = ref.grid_of(H, W)
    fwd, bwd = np.zeros((F, gh, gw, 2), np.int64), np.zeros((F, gh, gw, 2), np.int64)
    for u in range(F - 1):
        fwd[u] = tref.step_field(pyr[u], pyr[u + 1], kpyr[u], search, smooth)
        bwd[u + 1] = tref.step_field(pyr[u + 1], pyr[u], kpyr[u + 1], search, smooth)
    return fwd, bwd


def smooth_frames(images, known, fwd, bwd, radius, tolerance, frames=None):
    """The walk and the result for the frames `frames` (all by default) of the clip: (out fp32 [F, H, W, C], support int32
    [F, H, W]); frames not asked for keep the images and support -1 everywhere."""
    images = np.asarray(images, dtype=np.float32)
    F, H, W, C = images.shape
    w = weights(radius)
    out, support = images.copy(), np.full((F, H, W), -1, np.int32)
    V = {}

    def vectors(u, d):
        if (u, d) not in V:
            V[(u, d)] = ref.pixel_vectors((fwd if d == 1 else bwd)[u], H, W)
        return V[(u, d)]
    for t in (range(F) if frames is None else frames):
        ys, xs = np.nonzero(known[t] == 0)
        n = len(ys)
        x = images[t, ys, xs]                                             # [n, C]
        cx = ref.codes(x)
        acc = np.zeros((n, C), np.float32)
        total = np.full(n, w[0], np.int64)
        count = np.zeros(n, np.int32)
        for d in (-1, 1):
            alive = np.ones(n, bool)
            p = np.stack([16 * ys, 16 * xs], axis=-1).astype(np.int64)
            for k in range(1, radius + 1):
                u, v = t + (k - 1) * d, t + k * d
                if v < 0 or v >= F or not alive.any():
                    break
                i = (p + 8) >> 4                                          # a live p lies in the plane, and so does i
                q = p + vectors(u, d)[np.clip(i[:, 0], 0, H - 1), np.clip(i[:, 1], 0, W - 1)]
                alive &= (q[:, 0] >= 0) & (q[:, 0] <= 16 * (H - 1)) & (q[:, 1] >= 0) & (q[:, 1] <= 16 * (W - 1))
                s = tref.sample(images, np.full(n, v), q[:, 0], q[:, 1])  # of a dead chain: computed, never used
                alive &= np.abs(ref.codes(s) - cx).max(axis=1) <= tolerance
                with np.errstate(invalid="ignore", over="ignore"):
                    term = (np.float32(w[k]) * (s - x).astype(np.float32)).astype(np.float32)
                    acc = np.where(alive[:, None], (acc + term).astype(np.float32), acc)
                total += np.where(alive, w[k], 0)
                count += alive
                p = np.where(alive[:, None], q, p)
        with np.errstate(invalid="ignore", over="ignore"):
            new = (x + (acc / total.astype(np.float32)[:, None]).astype(np.float32)).astype(np.float32)
        out[t, ys, xs] = np.where((count > 0)[:, None], new, x)
        support[t, ys, xs] = count
    return out, support


def temporal_smooth_ref(images, mask, radius=2, tolerance=24, motion="background", levels=4, search=2, smooth=8):
    """The whole call: (out fp32 [F, H, W, C], support int32 [F, H, W])."""
    assert motion in MOTIONS
    images = np.asarray(images, dtype=np.float32)
    known = tref.known_bits(np.asarray(mask, dtype=np.float32), images.shape[0])
    fwd, bwd = fields(images, known, motion, levels, search, smooth)
    return smooth_frames(images, known, fwd, bwd, radius, tolerance)
