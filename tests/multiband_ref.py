"""The multiband blend's rule (include/lanpaint_hip.h, lp_multiband_blend) restated in numpy from the header's text: whole-level
array operations, no tiles.  dtype = np.float32 is the rule itself, every product, sum and difference rounded on its own (numpy
rounds every array operation); np.float64 is the same rule carried out more finely."""
import numpy as np

K5 = (0.0625, 0.25, 0.375, 0.25, 0.0625)


def level_sizes(H, W, levels):
    """[(h_0, w_0) .. (h_n, w_n)]: halved, rounded up, `levels` times or until (1, 1)."""
    sizes = [(int(H), int(W))]
    while len(sizes) <= levels and sizes[-1] != (1, 1):
        h, w = sizes[-1]
        sizes.append(((h + 1) // 2, (w + 1) // 2))
    return sizes


def reach(n):
    """No pixel further (Chebyshev) than this from every pixel with W_0 > 0 changes."""
    return 2 ** (n + 2) - 4


def weight0(mask, dtype=np.float32):
    m = np.asarray(mask, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(m > 0, np.minimum(m, np.float32(1)), np.float32(0)).astype(dtype)


def reduce_axis(x, axis):
    N = x.shape[axis]
    i = np.arange((N + 1) // 2)
    s = None
    for k, wgt in zip(range(-2, 3), K5):
        term = x.dtype.type(wgt) * np.take(x, np.clip(2 * i + k, 0, N - 1), axis=axis)
        s = term if s is None else s + term
    return s


def reduce(x):
    """[B, h, w, C] -> [B, ceil(h / 2), ceil(w / 2), C]: rows first over the full width, then columns."""
    return reduce_axis(reduce_axis(x, 1), 2)


def expand_axis(c, N, axis):
    T, n = c.dtype.type, c.shape[axis]
    i = np.arange(N)
    p = i // 2
    lo, mid, hi = (np.take(c, np.clip(q, 0, n - 1), axis=axis) for q in (p - 1, p, p + 1))
    even = T(0.125) * lo
    even = even + T(0.75) * mid
    even = even + T(0.125) * hi
    odd = T(0.5) * mid + T(0.5) * hi
    shape = [1] * c.ndim
    shape[axis] = N
    return np.where((i % 2 == 0).reshape(shape), even, odd)


def expand(c, h, w):
    """[B, h', w', C] -> [B, h, w, C]: rows first (giving [h, w']), then columns."""
    return expand_axis(expand_axis(c, h, 1), w, 2)


def blend_ref(image1, image2, mask, levels=5, dtype=np.float32):
    """image1, image2 [B, H, W, C], mask [Bm, H, W] with Bm in {1, B} -> [B, H, W, C] of `dtype`."""
    a, b = np.asarray(image1, dtype=np.float32).astype(dtype), np.asarray(image2, dtype=np.float32).astype(dtype)
    B, H, W, _ = a.shape
    sizes = level_sizes(H, W, levels)
    n = len(sizes) - 1
    D, Wt = [b - a], [weight0(mask, dtype)[..., None]]
    for _ in range(n):
        D.append(reduce(D[-1]))
        Wt.append(reduce(Wt[-1]))
    R = Wt[n] * D[n]
    for l in range(n - 1, -1, -1):
        h, w = sizes[l]
        lap = D[l] - expand(D[l + 1], h, w)
        R = expand(R, h, w) + Wt[l] * lap
    out = a + R
    assert out.dtype == dtype and out.shape == a.shape
    return out
