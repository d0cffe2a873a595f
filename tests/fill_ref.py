"""The push-pull fill and the outpaint canvas restated in numpy from the rule's text (include/lanpaint_hip.h, lp_mask_fill and
lp_outpaint_pad): whole-level array operations, one rounding per operation, no tiles, no spans.  `dtype` is the arithmetic's
type: np.float32 is the rule itself, np.float64 the same rule carried out more finely (to bound the rule's own rounding)."""
import numpy as np


def levels(H, W):
    out = [(H, W)]
    while out[-1] != (1, 1):
        h, w = out[-1]
        out.append(((h + 1) // 2, (w + 1) // 2))
    return out


def _pull(v, k):
    """One level up: v [h, w, C], k [h, w] bool -> (v', k') of (ceil(h / 2), ceil(w / 2))."""
    h, w, C = v.shape
    h2, w2 = (h + 1) // 2, (w + 1) // 2
    vp = np.zeros((2 * h2, 2 * w2, C), dtype=v.dtype)
    kp = np.zeros((2 * h2, 2 * w2), dtype=bool)                     # children outside the level are absent
    kp[:h, :w] = k
    vp[:h, :w] = np.where(k[..., None], v, 0)                       # a value whose flag is 0 is never used
    s = np.zeros((h2, w2, C), dtype=v.dtype)
    n = np.zeros((h2, w2), dtype=np.int32)
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        present = kp[dy::2, dx::2]
        s = np.where(present[..., None], s + vp[dy::2, dx::2], s)   # s = fl(s + v(child)), present children only
        n = n + present
    with np.errstate(invalid="ignore", divide="ignore"):
        out = s / n[..., None].astype(v.dtype)
    return np.where((n > 0)[..., None], out, 0).astype(v.dtype), n > 0


def _taps(n_fine, n_coarse, dtype):
    i = np.arange(n_fine)
    odd = (i % 2) == 1
    i0 = np.where(odd, (i - 1) // 2, i // 2 - 1)
    a0 = np.where(odd, 0.75, 0.25).astype(dtype)
    a1 = np.where(odd, 0.25, 0.75).astype(dtype)
    return np.clip(i0, 0, n_coarse - 1), np.clip(i0 + 1, 0, n_coarse - 1), a0, a1


def _up(f, h, w):
    """The 2x bilinear upsample of f [h', w', C] to [h, w, C], pixel centres aligned, taps clamped; rows first."""
    ty0, ty1, a0, a1 = _taps(h, f.shape[0], f.dtype)
    tx0, tx1, b0, b1 = _taps(w, f.shape[1], f.dtype)
    r = a0[:, None, None] * f[ty0] + a1[:, None, None] * f[ty1]    # [h, w', C]: two products, one sum, each rounded
    return b0[None, :, None] * r[:, tx0] + b1[None, :, None] * r[:, tx1]


def fill_one(image, mask, dtype=np.float32):
    """image [H, W, C], mask [H, W] -> [H, W, C]."""
    H, W, _ = image.shape
    known = ~(mask > 0.5)                                           # a NaN is not > 0.5: known
    v, k = [np.where(known[..., None], image, 0).astype(dtype)], [known]
    for _ in levels(H, W)[1:]:
        nv, nk = _pull(v[-1], k[-1])
        v.append(nv)
        k.append(nk)
    if not k[-1][0, 0]:
        return image.copy()
    f = v[-1]
    for l in range(len(v) - 2, -1, -1):
        f = np.where(k[l][..., None], v[l], _up(f, *v[l].shape[:2])).astype(dtype)
    return np.where(known[..., None], image, f.astype(image.dtype))


def fill_ref(image, mask, dtype=np.float32):
    """image [B, H, W, C] fp32, mask [Bm, H, W], Bm 1 or B -> [B, H, W, C]."""
    B = image.shape[0]
    return np.stack([fill_one(image[b], mask[b % mask.shape[0]], dtype) for b in range(B)])


def pad_ref(image, mask, left, top, right, bottom, overlap):
    """image [B, H, W, C], mask [Bm, H, W] or None -> (canvas [B, H', W', C], mask [max(Bm, 1), H', W'])."""
    B, H, W, C = image.shape
    Hc, Wc = top + H + bottom, left + W + right
    canvas = np.zeros((B, Hc, Wc, C), dtype=np.float32)
    canvas[:, top:top + H, left:left + W] = image
    band = np.ones((Hc, Wc), dtype=np.float32)
    y0, y1 = top + (overlap if top > 0 else 0), top + H - (overlap if bottom > 0 else 0)
    x0, x1 = left + (overlap if left > 0 else 0), left + W - (overlap if right > 0 else 0)
    band[max(y0, top):max(y1, top), max(x0, left):max(x1, left)] = 0.0
    Bm = 1 if mask is None else mask.shape[0]
    m = np.zeros((Bm, Hc, Wc), dtype=np.float32)
    if mask is not None:
        m[:, top:top + H, left:left + W] = mask
    return canvas, np.where(m > band[None], m, band[None]).astype(np.float32)      # a NaN m gives the band
