"""The mask refine's rule (include/lanpaint_hip.h, lp_mask_refine) restated in numpy from the header's text: whole-image array
operations, no tiles.  The integer stages are int64, the rest fp64, every operation rounded on its own (numpy rounds every array
operation), the sums of stage 3 in the header's order.  grow_ref states grow_mask's comparison on squared distances."""
import numpy as np


def codes(x):
    """fp32 values -> int64 codes 0..255: t = (v > 0) ? min(v, 1) : 0 (a NaN gives 0), (int)(t * 255.0f + 0.5f)."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        t = np.where(x > 0, np.minimum(x, np.float32(1)), np.float32(0)).astype(np.float32)
    return ((t * np.float32(255)).astype(np.float32) + np.float32(0.5)).astype(np.float32).astype(np.int64)


def _bounds(N, r):
    i = np.arange(N)
    return np.clip(i - r, 0, N), np.clip(i + r + 1, 0, N)


def box_int(a, r):
    """Exact window sums of an int64 plane [H, W], the (2r + 1)-square cut at the border."""
    H, W = a.shape
    ii = np.zeros((H + 1, W + 1), dtype=np.int64)
    ii[1:, 1:] = a.cumsum(0).cumsum(1)
    (y0, y1), (x0, x1) = _bounds(H, r), _bounds(W, r)
    return ii[y1][:, x1] - ii[y0][:, x1] - ii[y1][:, x0] + ii[y0][:, x0]


def count(H, W, r):
    (y0, y1), (x0, x1) = _bounds(H, r), _bounds(W, r)
    return ((y1 - y0)[:, None] * (x1 - x0)[None, :]).astype(np.int64)


def box_f64(a, r):
    """Stage 3's sums of an fp64 plane: over the window's columns in ascending x from +0.0, then over its rows in ascending y
    from +0.0; +0.0 stands for a term outside the image."""
    H, W = a.shape
    p = np.zeros((H, W + 2 * r), dtype=np.float64)
    p[:, r:r + W] = a
    h = np.zeros((H, W), dtype=np.float64)
    for k in range(2 * r + 1):
        h = h + p[:, k:k + W]
    p = np.zeros((H + 2 * r, W), dtype=np.float64)
    p[r:r + H] = h
    v = np.zeros((H, W), dtype=np.float64)
    for k in range(2 * r + 1):
        v = v + p[k:k + H]
    return v


def coefficients(G, P, r, eps):
    """Stages 1 and 2 of one image: G [H, W, 1 or 3] and P [H, W] int64 codes -> (a [H, W, 1 or 3], b [H, W]) as fp32."""
    H, W, C = G.shape
    f = np.float64
    n = count(H, W, r).astype(f)
    S = [box_int(G[..., c], r) for c in range(C)]
    Sp = box_int(P, r)
    Cv = [n * box_int(G[..., c] * P, r).astype(f) - S[c].astype(f) * Sp.astype(f) for c in range(C)]
    V = {(c, e): n * box_int(G[..., c] * G[..., e], r).astype(f) - S[c].astype(f) * S[e].astype(f)
         for c in range(C) for e in range(c, C)}
    R = (n * n) * (f(eps) * f(65025.0))
    S = [s.astype(f) for s in S]
    Sp = Sp.astype(f)
    with np.errstate(divide="ignore", invalid="ignore"):
        if C == 1:
            det = V[0, 0] + R
            a = [np.where(det > 0, Cv[0] / det, 0.0)]
            dot = a[0] * S[0]
        else:
            m00, m11, m22 = V[0, 0] + R, V[1, 1] + R, V[2, 2] + R
            m01, m02, m12 = V[0, 1], V[0, 2], V[1, 2]
            c00 = m11 * m22 - m12 * m12
            c01 = m02 * m12 - m01 * m22
            c02 = m01 * m12 - m02 * m11
            c11 = m00 * m22 - m02 * m02
            c12 = m01 * m02 - m00 * m12
            c22 = m00 * m11 - m01 * m01
            det = (m00 * c00 + m01 * c01) + m02 * c02
            ok = det > 0
            a = [np.where(ok, ((c00 * Cv[0] + c01 * Cv[1]) + c02 * Cv[2]) / det, 0.0),
                 np.where(ok, ((c01 * Cv[0] + c11 * Cv[1]) + c12 * Cv[2]) / det, 0.0),
                 np.where(ok, ((c02 * Cv[0] + c12 * Cv[1]) + c22 * Cv[2]) / det, 0.0)]
            dot = (a[0] * S[0] + a[1] * S[1]) + a[2] * S[2]
    b = (Sp - dot) / n
    return np.stack(a, axis=-1).astype(np.float32), b.astype(np.float32)


def refine_image(guide, mask, r, eps):
    """One image: guide [H, W, C] (C = 1 or >= 3), mask [H, W] -> [H, W] fp32."""
    guide = np.asarray(guide, dtype=np.float32)
    if guide.shape[-1] == 2:
        raise ValueError("a guide of two channels is refused")
    G = codes(guide[..., :1] if guide.shape[-1] < 3 else guide[..., :3])
    P = codes(mask)
    H, W, C = G.shape
    a, b = coefficients(G, P, r, eps)
    t = box_f64(a[..., 0].astype(np.float64), r) * G[..., 0].astype(np.float64)
    for c in range(1, C):
        t = t + box_f64(a[..., c].astype(np.float64), r) * G[..., c].astype(np.float64)
    t = t + box_f64(b.astype(np.float64), r)
    t = t / count(H, W, r).astype(np.float64)
    t = t / np.float64(255.0)
    return np.minimum(np.maximum(t, 0.0), 1.0).astype(np.float32)


def refine_ref(guide, mask, r, eps):
    """guide [B, H, W, C], mask [Bm, H, W] with Bm in {1, B} -> [B, H, W] fp32."""
    guide, mask = np.asarray(guide, dtype=np.float32), np.asarray(mask, dtype=np.float32)
    return np.stack([refine_image(guide[i], mask[0 if mask.shape[0] == 1 else i], r, eps) for i in range(guide.shape[0])])


D2_NONE = -1


def d2_brute(fg):
    """[H, W] bool -> int64 [2, H, W]: the squared Euclidean distance to the nearest True pixel and to the nearest False one,
    D2_NONE where there is none (what lp_vmask_edt returns), by comparing every pixel with every other."""
    H, W = fg.shape
    yy, xx = np.mgrid[:H, :W]
    out = np.full((2, H, W), D2_NONE, dtype=np.int64)
    for k, want in enumerate((fg, ~fg)):
        ys, xs = np.nonzero(want)
        if len(ys):
            out[k] = ((yy[..., None] - ys) ** 2 + (xx[..., None] - xs) ** 2).min(axis=-1)
    return out


def grow_ref(mask, grow):
    """grow_mask's rule on one [H, W] mask: the foreground is v >= 0.5; grow > 0: 1.0 where 0 <= d2_fg <= grow^2; grow < 0: 1.0
    where foreground and (d2_bg > grow^2 or there is no background); grow == 0: the mask itself."""
    mask = np.asarray(mask, dtype=np.float32)
    if grow == 0:
        return mask
    fg = mask >= np.float32(0.5)
    d2 = d2_brute(fg)
    if grow > 0:
        return ((d2[0] >= 0) & (d2[0] <= grow * grow)).astype(np.float32)
    return (fg & ((d2[1] > grow * grow) | (d2[1] == D2_NONE))).astype(np.float32)
