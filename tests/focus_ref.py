"""The focus form of lp_multiband_blend restated in numpy from the text of include/lanpaint_hip.h ("the focus form"): integers up
to the fit, fp64 with + - * / only in the fit, fp32 with every operation rounded on its own in the blur.  The constants are stated
again here, not imported; tests/test_focus_host.py holds them against the header.  Slow and plain on purpose."""
import math

import numpy as np

MAX_RING, MIN_COUNT, MAX_VAR, TILE, TAPS, HALO = 8, 64, 16, 32, 67, 5
NO_FIT = -1.0                                                          # the sigma^2 reported for a side that fits nothing
B8 = np.array([1, 8, 28, 56, 70, 56, 28, 8, 1], np.int64)
B2 = np.array([1, 2, 1], np.int64)


def mode_word(edge, ring, strength16, per_frame):
    u = 0x80000000 | edge | ring << 8 | strength16 << 12 | per_frame << 17
    return u - (1 << 32)


def codes_of(v):
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        t = np.where(v > 0, np.where(v < 1, v, np.float32(1)), np.float32(0)).astype(np.float32)      # a NaN gives 0
    return (t * np.float32(255) + np.float32(0.5)).astype(np.int64)


def luma(img):
    """[H, W, C] fp32 -> the 8-bit luma [H, W] as int64."""
    c = codes_of(img)
    if img.shape[-1] >= 3:
        return (77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8
    return c[..., 0]


def _sep(y, k):
    """The separable unnormalised filter on the valid part: [H, W] -> [H - n + 1, W - n + 1]."""
    n = len(k)
    h = sum(k[i] * y[:, i:y.shape[1] - n + 1 + i] for i in range(n))
    return sum(k[i] * h[i:h.shape[0] - n + 1 + i] for i in range(n))


def gradients(y):
    """(gA^2, gB^2) as int64 at the pixels whose 11 x 11 support lies inside the image: [H - 10, W - 10]."""
    a = _sep(y[3:-3, 3:-3], B2)                                        # A at the pixels 4 .. H - 5: one pixel around the valid ones
    b = _sep(y, B8)
    out = []
    for p in (a, b):
        gx, gy = p[1:-1, 2:] - p[1:-1, :-2], p[2:, 1:-1] - p[:-2, 1:-1]
        out.append(gx * gx + gy * gy)
    return out


def masked_of(mask):
    with np.errstate(invalid="ignore"):
        return np.asarray(mask, np.float32) > np.float32(0.5)          # a NaN is not masked


def tile_flags(masked):
    H, W = masked.shape
    th, tw = -(-H // TILE), -(-W // TILE)
    f = np.zeros((th, tw), bool)
    for ty in range(th):
        for tx in range(tw):
            f[ty, tx] = masked[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE].any()
    return f


def regions(mask, ring):
    """(ring, inside) as bool [H - 10, W - 10] over the pixels with their support inside the image."""
    masked = masked_of(mask)
    H, W = masked.shape
    win = np.lib.stride_tricks.sliding_window_view(masked, (11, 11))
    none, every = ~win.any((2, 3)), win.all((2, 3))
    f = tile_flags(masked)
    near = np.zeros_like(f)
    for ty, tx in np.argwhere(f):
        near[max(ty - ring, 0):ty + ring + 1, max(tx - ring, 0):tx + ring + 1] = True
    near_px = np.repeat(np.repeat(near, TILE, 0), TILE, 1)[HALO:H - HALO, HALO:W - HALO]
    return none & near_px, every


def stats_of(image1, image2, mask, edge, ring):
    """int64 [B, 2, 3]: per image (ring read on image2, inside read on image1) {n, sum gA^2, sum floor(gB^2 / 65536)}."""
    B, H, W, _ = image1.shape
    out = np.zeros((B, 2, 3), np.int64)
    if H < 11 or W < 11:
        return out
    thr = (edge * 2 * 65536) ** 2
    for b in range(B):
        reg = regions(mask[0 if mask.shape[0] == 1 else b], ring)
        for side, img in enumerate((image2, image1)):
            ga, gb = gradients(luma(img[b]))
            use = reg[side] & (gb >= thr)
            out[b, side] = int(use.sum()), int(ga[use].sum()), int((gb[use] >> 16).sum())
    return out


def variance_of(n, sa, sb):
    """sigma^2 of one side in fp64, every operation rounded on its own; NO_FIT under MIN_COUNT."""
    if n < MIN_COUNT:
        return np.float64(NO_FIT)
    a = np.float64(sa) / np.float64(256.0)
    b = np.float64(sb) / np.float64(65536.0)
    r = a / b
    q = r * r
    if not q > np.float64(1.0):
        return np.float64(MAX_VAR)
    return (np.float64(2.0) - np.float64(0.5) * q) / (q - np.float64(1.0))


def taps_of(K):
    """fp32 [67]: w(i) at index 33 + i."""
    k, t = K >> 4, K & 15
    w = np.zeros(TAPS, np.float32)
    for i in range(-(k + 1), k + 2):
        j = abs(i)
        # the coefficient to fp64 (round to nearest even), then an exact scaling by a power of two
        b0 = np.float64(math.ldexp(float(math.comb(2 * k, k + j)), -2 * k)) if j <= k else np.float64(0.0)
        b1 = np.float64(math.ldexp(float(math.comb(2 * k + 2, k + 1 + j)), -2 * k - 2))
        w[33 + i] = np.float32((np.float64(16 - t) * b0 + np.float64(t) * b1) / np.float64(16.0))
    return w


def fit(stats, strength16, per_frame):
    """-> (sigma2 fp64 [B, 2], K int32 [B], taps fp32 [B, 67])."""
    B = stats.shape[0]
    sig, K, taps = np.zeros((B, 2), np.float64), np.zeros(B, np.int32), np.zeros((B, TAPS), np.float32)
    pooled = stats.sum(0)
    for b in range(B):
        s = stats[b] if per_frame else pooled
        sig[b] = [variance_of(*map(int, s[side])) for side in (0, 1)]
        if s[0, 0] >= MIN_COUNT and s[1, 0] >= MIN_COUNT:
            d = sig[b, 0] - sig[b, 1]
            d = d if d > 0 else np.float64(0.0)
            v = (np.float64(strength16) / np.float64(16.0)) * d
            v = v if v < MAX_VAR else np.float64(MAX_VAR)
            K[b] = int(np.floor(v * np.float64(32.0) + np.float64(0.5)))
        taps[b] = taps_of(int(K[b]))
    return sig, K, taps


def weight0(mask):
    m = np.asarray(mask, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(m > 0, np.where(m < 1, m, np.float32(1)), np.float32(0)).astype(np.float32)


def blur(img, K, w):
    """The separable blur of one image [H, W, C] with the taps of K: rows first, coordinates clamped, fp32 op by op."""
    k, t = K >> 4, K & 15
    r = k + (1 if t else 0)
    v = np.asarray(img, np.float32)
    for axis in (1, 0):
        pad = [(0, 0)] * 3
        pad[axis] = (r, r)
        p = np.pad(v, pad, mode="edge")
        n = v.shape[axis]
        s = None
        for i in range(-r, r + 1):
            term = w[33 + i] * np.take(p, range(i + r, i + r + n), axis)
            s = term if s is None else s + term
        v = s.astype(np.float32)
    return v


def apply(image1, mask, K, taps):
    out = np.array(image1, np.float32, copy=True)
    for b in range(image1.shape[0]):
        if K[b] == 0:
            continue
        m = weight0(mask[0 if mask.shape[0] == 1 else b])[..., None]
        a = image1[b]
        got = a + m * (blur(a, int(K[b]), taps[b]) - a)
        out[b] = np.where(m > 0, got, a)
    return out


def match_focus_ref(image1, image2, mask, edge=8, ring=2, strength16=16, per_frame=0):
    """-> (out fp32 [B, H, W, C], stats int64 [B, 2, 3], sigma2 fp64 [B, 2], K int32 [B], taps fp32 [B, 67])."""
    image1, image2, mask = (np.asarray(a, np.float32) for a in (image1, image2, mask))
    stats = stats_of(image1, image2, mask, edge, ring)
    sig, K, taps = fit(stats, strength16, per_frame)
    return apply(image1, mask, K, taps), stats, sig, K, taps
