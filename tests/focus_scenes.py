"""Synthetic scenes for the focus match tests: a Voronoi image of random grey cells (the scene the estimator was prototyped on), a
float64 Gaussian blur, and a striped scene whose blur outside the mask steers the fitted K to a chosen value.  Numpy only."""
import functools

import numpy as np


def voronoi(seed, n=192, cells=60):
    """[n, n] float64 grey levels 0..255: every pixel takes the grey of the nearest of `cells` random points."""
    rng = np.random.default_rng(seed)
    pts = rng.random((cells, 2)) * n
    grey = rng.integers(0, 256, cells)
    yy, xx = np.mgrid[0:n, 0:n]
    d = (yy[..., None] - pts[:, 0]) ** 2 + (xx[..., None] - pts[:, 1]) ** 2
    return grey[d.argmin(-1)].astype(np.float64)


def gauss(img, sigma):
    """`img` [H, W] through a Gaussian of `sigma` pixels in float64, reflected at the border."""
    if sigma <= 0:
        return img.copy()
    r = int(np.ceil(5 * sigma))
    x = np.arange(-r, r + 1, dtype=np.float64)
    k = np.exp(-x * x / (2 * sigma * sigma))
    k /= k.sum()
    p = np.pad(img, r, mode="reflect")
    h = sum(k[i] * p[:, i:i + img.shape[1]] for i in range(2 * r + 1))
    return sum(k[i] * h[i:i + img.shape[0]] for i in range(2 * r + 1))


def quantised(levels):
    """grey levels 0..255 -> fp32 in 0..1 on exact 8-bit codes"""
    return (np.floor(levels + 0.5) / 255.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def soft_around_sharp(seed, sigma, n=192, box=(48, 144)):
    """(image [1, n, n, 1], mask [1, n, n]): the Voronoi scene blurred by `sigma` everywhere but sharp under the central mask."""
    sharp = voronoi(seed, n)
    scene = gauss(sharp, sigma)
    lo, hi = box
    scene[lo:hi, lo:hi] = sharp[lo:hi, lo:hi]
    mask = np.zeros((1, n, n), np.float32)
    mask[0, lo:hi, lo:hi] = 1.0
    img = quantised(scene)[None, :, :, None]
    img.setflags(write=False)
    mask.setflags(write=False)
    return img, mask


@functools.lru_cache(maxsize=None)
def stripes(sigma, n=128, period=32, box=(24, 104), channels=1, hi=215.0):
    """(image1, image2 [1, n, n, channels], mask [1, n, n]): vertical steps between grey 40 and `hi` every `period` pixels; image2
    is blurred by `sigma`, image1 is image2 with the sharp steps under the mask."""
    x = np.arange(n)
    sharp = np.where((x // period) % 2 == 0, 40.0, float(hi))[None, :].repeat(n, 0)
    soft = gauss(sharp, sigma)
    a0, a1 = box
    one = soft.copy()
    one[a0:a1, a0:a1] = sharp[a0:a1, a0:a1]
    mask = np.zeros((1, n, n), np.float32)
    mask[0, a0:a1, a0:a1] = 1.0
    out = []
    for a in (one, soft):
        a = np.ascontiguousarray(quantised(a)[None, :, :, None].repeat(channels, 3))
        a.setflags(write=False)
        out.append(a)
    mask.setflags(write=False)
    return out[0], out[1], mask
