"""Inputs the image-space tests share: images, masks and tables by seed.  numpy only, no device."""
import zlib

import numpy as np

from tests import grain_ref as ref


# (name, B, H, W, C, mask frames, rectangles (frame, y0, y1, x0, x1), soft seed, context, padding)
STITCH_CASES = [
    ("touching_region_edge", 2, 96, 128, 3, 2, [(0, 24, 55, 32, 63), (1, 24, 55, 32, 63)], None, 1.0, 0),
    ("flush_with_corner", 1, 96, 128, 3, 1, [(0, 0, 15, 104, 127)], None, 1.0, 0),
    ("flush_with_border_soft", 2, 90, 130, 4, 2, [(0, 30, 52, 0, 20), (1, 70, 89, 5, 30)], 3, 1.0, 0),
    ("one_mask_for_three_frames", 3, 96, 128, 3, 1, [(0, 40, 60, 50, 90)], 4, 1.5, 4),
    ("small_region", 1, 64, 64, 1, 1, [(0, 30, 33, 28, 35)], None, 1.0, 0),
]


def _rng(*key):
    return np.random.default_rng(list(key))


def _images(B, H, W, C, seed):
    rng = _rng(B, H, W, C, seed)
    r = rng.random((B, H, W, C), dtype=np.float32)
    d = (r * np.float32(0.9)).astype(np.float32) + rng.normal(0.03, 0.02, (B, H, W, C)).astype(np.float32)
    return d, r


def _blob_mask(Bm, H, W, seed):
    """Soft blobs: values on both sides of 0.5 with a gradual edge, a little noise on top."""
    rng = _rng(Bm, H, W, seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    m = np.zeros((Bm, H, W), dtype=np.float32)
    for p in range(Bm):
        for _ in range(2):
            cy, cx, s = rng.uniform(0, H), rng.uniform(0, W), 1.0 + min(H, W) / 8.0 * rng.uniform(0.5, 1.5)
            m[p] += np.float32(0.9) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / np.float32(2 * s * s)).astype(np.float32)
    return np.clip(m + rng.uniform(0, 0.05, m.shape).astype(np.float32), 0, 1).astype(np.float32)


def _boxes_ref(mask):
    """Per plane, in numpy: inclusive bounds of mask > 0.5, (H, -1, W, -1) for an empty plane."""
    m = mask.cpu().numpy()
    m = m[None] if m.ndim == 2 else m
    out = []
    for plane in m:
        ys, xs = np.nonzero(plane > np.float32(0.5))
        out.append((plane.shape[0], -1, plane.shape[1], -1) if ys.size == 0 else
                   (int(ys.min()), int(ys.max()), int(xs.min()), int(xs.max())))
    return tuple(out)


def _image(B, H, W, C, seed=0):
    return (np.float32(0.05) + np.float32(0.95) * _rng(B, H, W, C, seed).random((B, H, W, C), dtype=np.float32)).astype(np.float32)


def _fill_speckle(Bm, H, W, seed=1):
    return (_rng(Bm, H, W, seed).random((Bm, H, W)) < 0.3).astype(np.float32)


def _band(Bm, H, W):
    m = np.zeros((Bm, H, W), dtype=np.float32)
    m[:, :H // 4] = 1.0
    m[:, :, W - W // 3:] = 1.0
    return m


def _named_rng(*key):
    return np.random.default_rng([zlib.crc32(k.encode()) if isinstance(k, str) else int(k) for k in key])


def _noisy(size):
    def make(B, H, W, C, seed=1):
        rng = _named_rng(B, H, W, C, size, seed)
        ramp = np.linspace(0.2, 0.8, W)[None, None, :, None] + 0.02 * np.arange(C)[None, None, None, :] / max(C, 1)
        n = rng.normal(0.0, 1.0, (B, H + 4, W + 4, C))
        k = ref.KERNELS[size].astype(np.float64)
        f = np.zeros((B, H, W, C))
        for dy in range(-size, size + 1):
            for dx in range(-size, size + 1):
                f += k[dy + size, dx + size] * n[:, 2 + dy:2 + dy + H, 2 + dx:2 + dx + W]
        return (ramp + 0.03 * f / np.sqrt(ref.SUM_K2[size])).astype(np.float32)
    return make


def _checker(B, H, W, C, seed=0):
    yy, xx = np.mgrid[:H, :W]
    return np.broadcast_to(((yy + xx) & 1).astype(np.float32)[None, :, :, None], (B, H, W, C)).copy()


def _boundaries(B, H, W, C, seed=2):
    """(k + 0.5) / 255 and its float neighbours, where the code changes."""
    rng = _named_rng(B, H, W, C, seed)
    v = ((rng.integers(0, 255, (B, H, W, C)) + 0.5) / 255.0).astype(np.float32)
    step = rng.integers(-1, 2, (B, H, W, C))
    return np.where(step < 0, np.nextafter(v, np.float32(0)), np.where(step > 0, np.nextafter(v, np.float32(1)), v)).astype(np.float32)


def _grain_wild(B, H, W, C, seed=3):
    """NaN, infinities and values outside [0, 1]."""
    rng = _named_rng(B, H, W, C, seed)
    m = (1.6 * rng.random((B, H, W, C)) - 0.3).astype(np.float32)
    pick = rng.random((B, H, W, C))
    m[pick < 0.05] = np.nan
    m[(pick >= 0.05) & (pick < 0.08)] = np.inf
    m[(pick >= 0.08) & (pick < 0.11)] = -np.inf
    return m


IMAGES = {"white": _noisy(0), "medium": _noisy(1), "coarse": _noisy(2), "all 0": lambda *s: np.zeros(s, np.float32),
          "all 1": lambda *s: np.ones(s, np.float32), "checker": _checker, "boundaries": _boundaries, "wild": _grain_wild}


def _box(B, H, W, per_image=True):
    m = np.zeros((B if per_image else 1, H, W), np.float32)
    for i in range(m.shape[0]):
        m[i, H // 5 + i % 3:H - H // 5, W // 6 + i % 2:W - W // 4] = 1.0
    return m


def _m3(mask):
    return mask[None] if mask.ndim == 2 else mask


def _random_table(B, C, seed, scale=400):
    rng = _named_rng(B, C, seed)
    n = rng.integers(0, 200, (B, C, ref.K))
    n[rng.random((B, C, ref.K)) < 0.3] = 0
    e1 = (n * rng.random((B, C, ref.K)) * scale).astype(np.int64)
    e2 = (n * rng.random((B, C, ref.K)) * scale * rng.choice([1, 20, 50], (B, 1, 1))).astype(np.int64)
    return np.stack([n, e1, e2], axis=-1).astype(np.int64)


def _soft(Bm, H, W, seed=1):
    return _rng(Bm, H, W, seed).random((Bm, H, W), dtype=np.float32)


def _multiband_speckle(Bm, H, W, seed=2):
    return (_rng(Bm, H, W, seed).random((Bm, H, W)) < 0.3).astype(np.float32)


def _guide(B, H, W, C, seed=0):
    """Two flat regions with noise, so that windows see an edge; values run a little outside [0, 1]."""
    rng = _rng(B, H, W, C, seed)
    yy, xx = np.mgrid[:H, :W]
    side = ((xx - W / 2) + 0.4 * (yy - H / 2) < 0)[None, :, :, None]
    base = np.where(side, rng.random((B, 1, 1, C)), rng.random((B, 1, 1, C)))
    return (base + rng.normal(0, 0.08, (B, H, W, C))).astype(np.float32)


def _refine_blobs(Bm, H, W, seed=2):
    yy, xx = np.mgrid[:H, :W]
    m = ((xx - W / 2 + 3 * np.sin(yy / 3.0)) + 0.4 * (yy - H / 2) < 2).astype(np.float32)
    m = np.repeat(m[None], Bm, axis=0)
    m[:, H // 3:H // 3 + 3, W // 4:W // 4 + 5] = 1.0 - m[:, H // 3:H // 3 + 3, W // 4:W // 4 + 5]
    return m


def _stabilize_soft(F, H, W, seed=1):
    return _rng(F, H, W, seed).random((F, H, W), dtype=np.float32)


def _stabilize_blobs(F, H, W, seed=2):
    """A disc that drifts and jitters, an empty frame and a stray blob in it."""
    rng = _rng(F, H, W, seed)
    yy, xx = np.mgrid[:H, :W]
    m = np.zeros((F, H, W), dtype=np.float32)
    for t in range(F):
        cy, cx = H / 2 + rng.normal(0, 1), W / 3 + 0.7 * t + rng.normal(0, 1)
        m[t] = (yy - cy) ** 2 + (xx - cx) ** 2 <= (min(H, W) / 3 + rng.normal(0, 1)) ** 2
    m[F // 3] = 0.0
    m[F // 2, :2, -3:] = 1.0
    return m


def _alternating(F, H, W):
    m = np.zeros((F, H, W), dtype=np.float32)
    m[1::2] = 1.0
    return m


def _single(F, H, W):
    m = np.zeros((F, H, W), dtype=np.float32)
    m[F // 2, H // 2, W // 3] = 1.0
    return m


def _threshold(F, H, W, seed=3):
    """0.5 and its float neighbours."""
    v = np.float32(0.5)
    return _rng(F, H, W, seed).choice(np.array([np.nextafter(v, np.float32(0)), v, np.nextafter(v, np.float32(1))]), (F, H, W))


def _stabilize_wild(F, H, W, seed=4):
    """NaN, infinities and values outside [0, 1]."""
    rng = _rng(F, H, W, seed)
    m = (3.0 * rng.random((F, H, W)) - 1.0).astype(np.float32)
    pick = rng.random((F, H, W))
    m[pick < 0.15] = np.nan
    m[(pick >= 0.15) & (pick < 0.2)] = np.inf
    m[(pick >= 0.2) & (pick < 0.25)] = -np.inf
    return m


FORMS = {"soft": _stabilize_soft, "blobs": _stabilize_blobs, "all 0": lambda *s: np.zeros(s, np.float32),
         "all 1": lambda *s: np.ones(s, np.float32), "alternating": _alternating, "single": _single, "threshold": _threshold, "wild": _stabilize_wild}


def _blob(rng, h, w):
    """A soft mask in [0, 1]: two Gaussian bumps, the larger one deep enough inside the frame to have an interior."""
    yy, xx = np.mgrid[:h, :w].astype(np.float64)
    s = 0.25 * min(h, w) + 0.5
    f = np.zeros((h, w))
    for scale in (1.0, 0.5):
        cy, cx = rng.uniform(0.35, 0.65) * h, rng.uniform(0.1, 0.9) * w
        f += np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * (s * scale) ** 2))
    return np.clip(f, 0.0, 1.0).astype(np.float32)


def _keys(rng, h, w):
    """Five keys: two soft blobs, one whose foreground is exactly 0.5 next to nextafter(0.5, 0), one empty, one full."""
    half, below = np.float32(0.5), np.nextafter(np.float32(0.5), np.float32(0))
    edge = np.where(_blob(rng, h, w) >= 0.4, half, below).astype(np.float32)
    edge[rng.random((h, w)) < 0.02] = 1.0
    edge[rng.random((h, w)) < 0.02] = 0.0
    return np.stack([_blob(rng, h, w), _blob(rng, h, w), edge, np.zeros((h, w), np.float32), np.ones((h, w), np.float32)])


def _row(kind, lo=0, hi=0, sy1=0, sx1=0, sy2=0, sx2=0, wf=0.0):
    return (kind, lo, hi, sx1, sy1, sx2, sy2, 0, wf, 1.0 - wf)


def _apply(codes, bx, kx, by, ky):
    """The two integer passes the kernel runs, one numpy loop per output index (Pillow's ImagingResampleHorizontal_8bpc /
    ImagingResampleVertical_8bpc)."""
    h, _ = codes.shape
    tmp = np.empty((h, len(bx)), np.int64)
    for xx, (x0, n) in enumerate(bx):
        ss = (1 << 21) + codes[:, x0:x0 + n].astype(np.int64) @ kx[xx, :n].astype(np.int64)
        tmp[:, xx] = np.clip(ss >> 22, 0, 255)
    out = np.empty((len(by), len(bx)), np.int64)
    for yy, (y0, n) in enumerate(by):
        ss = (1 << 21) + ky[yy, :n].astype(np.int64) @ tmp[y0:y0 + n]
        out[yy] = np.clip(ss >> 22, 0, 255)
    return out.astype(np.uint8)


def _pairs():
    rng = np.random.default_rng(3)
    pairs = [((832, 480), (1280, 720)), ((7, 9), (3, 400)), ((56, 40), (97, 61)), ((56, 40), (23, 17)), ((45, 31), (19, 53)),
             ((10, 10), (10, 17)), ((13, 9), (40, 9)), ((1, 5), (7, 1)), ((300, 2), (1, 1))]
    while len(pairs) < 32:
        w, h = (int(v) for v in rng.integers(1, 200, 2))
        ow, oh = (int(v) for v in rng.integers(1, 300, 2))
        pairs.append(((w, h), (ow, oh)))
    return pairs
