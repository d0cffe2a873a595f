"""The video mask stabilize restated in numpy (tests/test_stabilize_host.py, tests/test_gpu_stabilize.py): the rule of
include/lanpaint_hip.h (lp_mask_signed_d2, lp_mask_stabilize) in int64 and float64, every product and every sum a numpy operation
of its own, the sums in the order the rule names.  The squared distances come from the exact integer EDT of
tests/videomask_ref.py.  Nothing here touches a device.
"""
import math

import numpy as np

from tests import videomask_ref

Q_FAR = 1 << 30
SD_CAP = 64.0


def d2_exact(on):
    """[H, W] bool -> int64 [H, W]: the squared Euclidean distance of every True pixel to the nearest False pixel, 0 on False
    pixels.  `on` must hold a False pixel.  videomask_ref.edt_numpy forms the exact integer and returns its square root; an
    integer below 2^53 comes back from squaring that and rounding."""
    return np.rint(videomask_ref.edt_numpy(on) ** 2).astype(np.int64)


def signed_d2_frame(frame):
    """Stage 1 for one [H, W] fp32 frame: int64 [H, W]."""
    fg = np.asarray(frame, dtype=np.float32) >= np.float32(0.5)          # a NaN compares false: background
    if not fg.any():
        return np.full(fg.shape, -Q_FAR, dtype=np.int64)
    if fg.all():
        return np.full(fg.shape, Q_FAR, dtype=np.int64)
    return np.where(fg, d2_exact(fg), -d2_exact(~fg))


def signed_d2(mask):
    """Stage 1: [F, H, W] fp32 -> int64 [F, H, W]."""
    return np.stack([signed_d2_frame(f) for f in np.asarray(mask, dtype=np.float32)])


def signed_from_planes(d2):
    """lp_mask_signed_d2 on lp_vmask_edt's planes: int [F, 2, H, W] -> int64 [F, H, W]."""
    d2 = np.asarray(d2, dtype=np.int64)
    fg_d, bg_d = d2[:, 0], d2[:, 1]
    return np.where(fg_d == 0, np.where(bg_d == -1, Q_FAR, bg_d), np.where(fg_d == -1, -Q_FAR, -fg_d))


def _at(a, t):
    """a[clamp(t, 0, F - 1)] for every frame index of `t`."""
    return a[np.clip(t, 0, a.shape[0] - 1)]


def temporal_median(q, tm):
    """Stage 2: the median of q[clamp(t + k)], k = -tm..tm, per pixel; int64."""
    F = q.shape[0]
    t = np.arange(F)
    window = np.stack([_at(q, t + k) for k in range(-tm, tm + 1)])       # [2 tm + 1, F, H, W]
    return np.sort(window, axis=0)[tm]


def capped_distance(qm):
    """Stage 3: sign(qm) * sqrt(|qm|) in float64, capped at +-SD_CAP."""
    s = np.sign(qm).astype(np.float64) * np.sqrt(np.abs(qm).astype(np.float64))
    return np.minimum(np.maximum(s, -SD_CAP), SD_CAP)


def temporal_smooth(s, ts):
    """Stage 4: the binomial sum over k = -ts..ts in ascending order from +0.0, then the division by 4^ts."""
    t = np.arange(s.shape[0])
    acc = np.zeros(s.shape, dtype=np.float64)
    for k in range(-ts, ts + 1):
        prod = np.float64(math.comb(2 * ts, ts + k)) * _at(s, t + k)
        acc = acc + prod
    return acc / np.float64(4 ** ts)


def output(sd, grow, feather):
    """Stage 5."""
    u = sd + np.float64(grow)
    if feather == 0:
        return (u > 0).astype(np.float32)
    v = np.float64(0.5) + u / (np.float64(2.0) * np.float64(feather))
    return np.minimum(np.maximum(v, 0.0), 1.0).astype(np.float32)


def stabilize_q_ref(q, median=1, smooth=2, grow=0.0, feather=0.0):
    """Stages 2 to 5 on signed squared distances [F, H, W]: fp32 [F, H, W]."""
    q = np.asarray(q, dtype=np.int64)
    return output(temporal_smooth(capped_distance(temporal_median(q, median)), smooth), grow, feather)


def stabilize_ref(mask, median=1, smooth=2, grow=0.0, feather=0.0):
    """The whole rule: mask [F, H, W] fp32 -> fp32 [F, H, W]."""
    return stabilize_q_ref(signed_d2(mask), median, smooth, grow, feather)
