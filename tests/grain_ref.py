"""The grain match (include/lanpaint_hip.h, lp_grain_*) restated in numpy: exact integers, then fp64 and fp32 with every
operation rounded on its own.  Philox4x32-10 is written out in uint64 arithmetic.  The device must give these bits."""
import numpy as np

from tests.refine_ref import codes

K, MIN_COUNT, WHITE_VAR, MAX_STD, MAX_MARGIN = 8, 64, 21845, 64, 25
ALL, OUTSIDE, INSIDE = 0, 1, 2
AUTO = -1
KERNELS = (np.array([[1]], dtype=np.int64),
           np.outer([1, 2, 1], [1, 2, 1]).astype(np.int64),
           np.outer([1, 4, 6, 4, 1], [1, 4, 6, 4, 1]).astype(np.int64))
B3 = KERNELS[1]
N3 = np.array([[1, -2, 1], [-2, 4, -2], [1, -2, 1]], dtype=np.int64)
N5 = np.zeros((5, 5), dtype=np.int64)
N5[::2, ::2] = N3
SUM_K2 = (1, 36, 4900)
S1 = (36, 36, 784)
S2 = (36, 784, 39204)
M32 = np.uint64(0xFFFFFFFF)


def full_conv(a, b):
    """The full 2-D convolution of two small integer kernels."""
    out = np.zeros((a.shape[0] + b.shape[0] - 1, a.shape[1] + b.shape[1] - 1), dtype=np.int64)
    for i in range(b.shape[0]):
        for j in range(b.shape[1]):
            out[i:i + a.shape[0], j:j + a.shape[1]] += b[i, j] * a
    return out


def philox4x32_10(ctr, subseq, seed):
    """Random123's Philox4x32-10: counter (ctr [64 bit], subseq [64 bit]), key seed [64 bit]; arrays broadcast.  Four uint64
    arrays holding the 32-bit words."""
    ctr, subseq, seed = (np.asarray(v, dtype=np.uint64) for v in (ctr, subseq, seed))
    ctr, subseq, seed = np.broadcast_arrays(ctr, subseq, seed)
    c0, c1, c2, c3 = ctr & M32, ctr >> np.uint64(32), subseq & M32, subseq >> np.uint64(32)
    k0, k1 = seed & M32, seed >> np.uint64(32)
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                                       # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def white_of(word):
    """The sum of a 32-bit word's four bytes, minus 510."""
    w = np.asarray(word, dtype=np.uint64)
    s = (w & np.uint64(255)) + ((w >> np.uint64(8)) & np.uint64(255)) + ((w >> np.uint64(16)) & np.uint64(255)) + (w >> np.uint64(24))
    return s.astype(np.int64) - 510


def white(frame, H, W, C, seed, monochrome=False):
    """w(frame, y, x, c) for -2 <= y < H + 2, -2 <= x < W + 2: int64 [H + 4, W + 4, C]."""
    yy, xx = np.mgrid[0:H + 4, 0:W + 4]
    ctr = (yy * (W + 4) + xx).astype(np.uint64)
    out = np.zeros((H + 4, W + 4, C), dtype=np.int64)
    for g in range(1 if monochrome else (C + 3) // 4):
        words = philox4x32_10(ctr, np.uint64(frame * 16 + g), np.uint64(seed))
        if monochrome:
            out[:] = white_of(words[0])[..., None]
        else:
            for j in range(min(4, C - 4 * g)):
                out[..., 4 * g + j] = white_of(words[j])
    return out


def grain_field(B, H, W, C, size, seed=0, monochrome=False, frame0=0):
    """g = sum k_s(dy, dx) w(y + dy, x + dx): int32 [B, H, W, C]."""
    k = KERNELS[size]
    out = np.zeros((B, H, W, C), dtype=np.int64)
    for i in range(B):
        w = white(frame0 + i, H, W, C, seed, monochrome)
        for dy in range(-size, size + 1):
            for dx in range(-size, size + 1):
                out[i] += k[dy + size, dx + size] * w[2 + dy:2 + dy + H, 2 + dx:2 + dx + W]
    return out.astype(np.int32)


def _window_all(ok, r):
    """ok [H, W] bool -> every element within r rows and columns, inside the image, is True."""
    H, W = ok.shape
    pad = np.ones((H + 2 * r, W + 2 * r), dtype=bool)
    pad[r:r + H, r:r + W] = ok
    out = np.ones((H, W), dtype=bool)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out &= pad[dy:dy + H, dx:dx + W]
    return out


def _correlate(q, k, pad):
    """sum k(dy, dx) q(y + dy, x + dx) over q [H, W] int64 padded by `pad` (an edge-replicated or a zero pad is the caller's)."""
    r = k.shape[0] // 2
    H, W = q.shape[0] - 2 * pad, q.shape[1] - 2 * pad
    out = np.zeros((H, W), dtype=np.int64)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if k[dy + r, dx + r]:
                out += k[dy + r, dx + r] * q[pad + dy:pad + dy + H, pad + dx:pad + dx + W]
    return out


def grain_stats(image, mask=None, region=ALL, flat=64, margin=8):
    """Stage 1: int64 [B, C, K, 3] = {n, sum e1^2, sum e2^2}.  image [B, H, W, C], mask [1 or B, H, W] or None."""
    image = np.asarray(image, dtype=np.float32)
    B, H, W, C = image.shape
    out = np.zeros((B, C, K, 3), dtype=np.int64)
    if H < 5 or W < 5:
        return out
    q = codes(image)
    inner = np.zeros((H, W), dtype=bool)
    inner[2:H - 2, 2:W - 2] = True
    for i in range(B):
        take = inner.copy()
        if region != ALL:
            m = np.asarray(mask, dtype=np.float32)
            m = m[0 if m.shape[0] == 1 else i]
            with np.errstate(invalid="ignore"):
                take &= _window_all(m <= np.float32(0.5), margin) if region == OUTSIDE else _window_all(m > np.float32(0.5), 2)
        for c in range(C):
            p = np.pad(q[i, :, :, c], 2)
            hi = np.full((H, W), -1, dtype=np.int64)
            lo = np.full((H, W), 256, dtype=np.int64)
            for dy in range(5):
                for dx in range(5):
                    hi = np.maximum(hi, p[dy:dy + H, dx:dx + W])
                    lo = np.minimum(lo, p[dy:dy + H, dx:dx + W])
            t = take & (hi - lo <= flat)
            mu16, e1, e2 = _correlate(p, B3, 2), _correlate(p, N3, 2), _correlate(p, N5, 2)
            band = (mu16 * K) // 4081
            for k in range(K):
                sel = t & (band == k)
                out[i, c, k] = (sel.sum(), (e1[sel] ** 2).sum(), (e2[sel] ** 2).sum())
    return out


def _fill(E, valid):
    """E [K] with every invalid band taking the nearest valid one's value, the lower index on a tie; None when none is valid."""
    idx = np.flatnonzero(valid)
    if idx.size == 0:
        return None
    out = E.copy()
    for k in range(K):
        best = min(idx, key=lambda j: (abs(int(j) - k), j))
        out[k] = E[best]
    return out


def grain_fit(gen, ref, strength=1.0, size=AUTO, clip_frames=0):
    """Stage 2: (amp fp32 [B, C, K], size int32 [B])."""
    gen, ref = np.asarray(gen, dtype=np.int64), np.asarray(ref, dtype=np.int64)
    B, C = gen.shape[:2]
    Br = ref.shape[0]
    L = clip_frames or B
    amp = np.zeros((B, C, K), dtype=np.float32)
    sizes = np.zeros(B, dtype=np.int32)
    strength = np.float64(strength)

    def pool(rows):
        acc = np.zeros(rows.shape[1:], dtype=np.float64)
        for r in rows:
            acc = acc + r.astype(np.float64)
        return acc

    for clip in range(B // L):
        lo = clip * L
        Pg = pool(gen[lo:lo + L])
        Pr = pool(ref[lo:lo + L] if Br == B else ref)
        need = np.zeros((2, C, K), dtype=np.float64)
        for c in range(C):
            E = []
            for P in (Pg, Pr):
                valid = P[c, :, 0] >= MIN_COUNT
                n = np.where(valid, P[c, :, 0], 1.0)
                E.append([_fill(np.where(valid, P[c, :, j] / n, 0.0), valid) for j in (1, 2)])
            if E[1][0] is None:
                continue
            for j in range(2):
                eg = E[0][j] if E[0][j] is not None else np.zeros(K)
                need[j, c] = np.maximum(0.0, E[1][j] - eg)
        s, none = size, False
        if size == AUTO:
            A = Bq = np.float64(0.0)
            for c in range(C):
                for k in range(K):
                    A = A + need[0, c, k]
                    Bq = Bq + need[1, c, k]
            if not A > 0:
                s, none = 0, True
            elif np.float64(3.0) * Bq < np.float64(14.0) * A:
                s = 0
            elif Bq < np.float64(33.0) * A:
                s = 1
            else:
                s = 2
        den = np.float64(WHITE_VAR * (S1[s] + S2[s]))
        a = strength * np.sqrt((need[0] + need[1]) / den)
        a = np.minimum(a, np.float64(MAX_STD) / np.sqrt(np.float64(WHITE_VAR * SUM_K2[s])))
        if none:
            a = np.zeros_like(a)
        amp[lo:lo + L] = (a / np.float64(255.0)).astype(np.float32)
        sizes[lo:lo + L] = s
    return amp, sizes


def mask01(mask):
    """(v > 0) ? min(v, 1) : 0; a NaN gives 0."""
    m = np.asarray(mask, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(m > 0, np.minimum(m, np.float32(1)), np.float32(0)).astype(np.float32)


def grain_apply(image, mask, amp, sizes, seed=0, monochrome=False, frame0=0):
    """Stage 3: fp32 [B, H, W, C]."""
    image = np.asarray(image, dtype=np.float32)
    B, H, W, C = image.shape
    q = codes(image)
    m = np.asarray(mask, dtype=np.float32)
    out = np.empty_like(image)
    f32 = np.float32
    for i in range(B):
        g = grain_field(1, H, W, C, int(sizes[i]), seed, monochrome, frame0 + i)[0].astype(np.float32)
        mi = mask01(m[0 if m.shape[0] == 1 else i])
        for c in range(C):
            mu16 = _correlate(np.pad(q[i, :, :, c], 1, mode="edge"), B3, 1)
            u = ((mu16 * K).astype(np.float32) / f32(4080.0)).astype(np.float32) - f32(0.5)
            u = np.minimum(np.maximum(u, f32(0)), f32(K - 1)).astype(np.float32)
            k0 = np.minimum(u.astype(np.int64), K - 2)
            f = (u - k0.astype(np.float32)).astype(np.float32)
            a0, a1 = amp[i, c][k0], amp[i, c][k0 + 1]
            a = (a0 + (f * (a1 - a0).astype(np.float32)).astype(np.float32)).astype(np.float32)
            t = (mi * a).astype(np.float32)
            x = image[i, :, :, c]
            with np.errstate(invalid="ignore", over="ignore"):
                o = (x + (t * g[:, :, c]).astype(np.float32)).astype(np.float32)
            res = np.where(t == 0, x, o)
            keep = (t == 0)
            resb = res.view(np.uint32).copy()
            resb[keep] = np.ascontiguousarray(x).view(np.uint32)[keep]   # the input's bits, a NaN's payload included
            out[i, :, :, c] = resb.view(np.float32)
    return out


def match(image, mask, reference=None, strength=1.0, size=AUTO, monochrome=False, flat=64, margin=8, seed=0, clip_frames=0,
          frame0=0):
    """lanpaint_amd.grain.match.  mask [1 or B, H, W]."""
    ref = grain_stats(reference, None, ALL, flat) if reference is not None else grain_stats(image, mask, OUTSIDE, flat, margin)
    gen = grain_stats(image, mask, INSIDE, flat)
    amp, sizes = grain_fit(gen, ref, strength, size, clip_frames)
    return grain_apply(image, mask, amp, sizes, seed, monochrome, frame0)
