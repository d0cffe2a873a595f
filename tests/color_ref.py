"""The Detailer colour match restated in numpy, from the rule in lanpaint_amd/detail_color.py's docstring and not from the
kernel: the keep mask from scipy's maximum_filter, the sums from math.fsum (correctly rounded whatever the order), the fit in
float64 one operation at a time, the affine map in float32."""
import math

import numpy as np
from scipy import ndimage

MIN_COUNT = 64


def keep_mask(mask, margin, batch, H, W):
    """bool [batch, H, W]: pixel kept <=> every mask element within `margin` rows and columns, inside the image, is <= 0.5."""
    if mask is None:
        return np.ones((batch, H, W), dtype=bool)
    m = np.asarray(mask, dtype=np.float32)
    if m.ndim == 2:
        m = m[None]
    assert m.shape[0] in (1, batch) and m.shape[1:] == (H, W)
    over = (~(m <= np.float32(0.5))).astype(np.uint8)
    k = 2 * margin + 1
    near = ndimage.maximum_filter(over, size=(1, k, k), mode="constant", cval=0)      # outside the image: does not count
    return np.broadcast_to(near == 0, (batch, H, W))


def stats_ref(detail, reference, mask, margin):
    """(stats float64 [B, 1 + 4 C], bound float64 [B, 1 + 4 C]): the sums by math.fsum, and for each the sum of |term| that the
    error bound of a plain fp64 summation is stated in.  Terms are exact in float64: a float32, or the square of one."""
    d, r = np.asarray(detail, dtype=np.float32).astype(np.float64), np.asarray(reference, dtype=np.float32).astype(np.float64)
    B, H, W, C = d.shape
    keep = keep_mask(mask, margin, B, H, W)
    stats, mag = np.zeros((B, 1 + 4 * C)), np.zeros((B, 1 + 4 * C))
    for i in range(B):
        stats[i, 0] = int(keep[i].sum())
        for c in range(C):
            dk, rk = d[i, :, :, c][keep[i]], r[i, :, :, c][keep[i]]
            for j, terms in enumerate((dk, rk, dk * dk, rk * rk)):
                stats[i, 1 + 4 * c + j] = math.fsum(terms.tolist())
                mag[i, 1 + 4 * c + j] = math.fsum(np.abs(terms).tolist())
    return stats, mag


def fit_ref(stats, method="mean_std", strength=1.0, smooth=1, clip_frames=0):
    """float32 [B, C, 2] = (gain, bias) from stats float64 [B, 1 + 4 C]."""
    stats = np.asarray(stats, dtype=np.float64)
    B, C = stats.shape[0], (stats.shape[1] - 1) // 4
    L = clip_frames or B
    assert B % L == 0 and (smooth == 0 or smooth % 2 == 1) and method in ("mean", "mean_std")
    s = np.float64(strength)
    coef = np.zeros((B, C, 2), dtype=np.float32)
    for i in range(B):
        q, f = divmod(i, L)
        lo, hi = (0, L - 1) if smooth == 0 else (max(0, f - smooth // 2), min(L - 1, f + smooth // 2))
        P = np.zeros(stats.shape[1])
        for g in range(lo, hi + 1):
            P = P + stats[q * L + g]                               # one rounded add per entry, ascending frames
        N = P[0]
        for c in range(C):
            if N < MIN_COUNT:
                coef[i, c] = (1.0, 0.0)
                continue
            sd, sr, sdd, srr = P[1 + 4 * c: 5 + 4 * c]
            md, mr = sd / N, sr / N
            vd = sdd / N - md * md
            vr = srr / N - mr * mr
            g = np.float64(1.0)
            if method == "mean_std" and not (vd <= 1e-8) and vr >= 0.0:
                g = np.sqrt(vr / vd)
                g = np.float64(0.25) if g < 0.25 else np.float64(4.0) if g > 4.0 else g
            b = mr - g * md
            coef[i, c, 0] = np.float32(np.float64(1.0) + s * (g - np.float64(1.0)))
            coef[i, c, 1] = np.float32(s * b)
    return coef


def apply_ref(detail, coef):
    """float32 (d * gain) rounded, + bias rounded."""
    d = np.asarray(detail, dtype=np.float32)
    k = np.asarray(coef, dtype=np.float32)
    g, b = k[:, None, None, :, 0], k[:, None, None, :, 1]
    return (d * g).astype(np.float32) + b


def match_ref(detail, reference, mask, method="mean_std", strength=1.0, margin=8, smooth=1, clip_frames=0):
    stats, _ = stats_ref(detail, reference, mask, margin)
    return apply_ref(detail, fit_ref(stats, method, strength, smooth, clip_frames))
