"""numpy restatement of the video mask propagate rule, written from include/lanpaint_hip.h (lp_prop_*): every stage and the whole
chain in integers.  A block-matching motion field from frame s to the next frame t, weighted by the mask of s, carries a map of
key-frame positions along; the key mask is sampled through that map.  Nothing here looks at the kernels."""
import numpy as np

BLOCK, HALO, MIN_PIXELS, FILL_ITERS = 8, 4, 16, 3


def codes(x):
    """fp32 values -> int64 codes 0..255: t = (v > 0) ? min(v, 1) : 0 (a NaN gives 0), (int)(t * 255.0f + 0.5f), no FMA."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        t = np.where(x > 0, np.minimum(x, np.float32(1)), np.float32(0)).astype(np.float32)
    return ((t * np.float32(255)).astype(np.float32) + np.float32(0.5)).astype(np.float32).astype(np.int64)


def luma(images):
    """fp32 [F, H, W, C] -> uint8 [F, H, W]."""
    q = codes(images)
    if q.shape[-1] >= 3:
        return ((77 * q[..., 0] + 150 * q[..., 1] + 29 * q[..., 2] + 128) >> 8).astype(np.uint8)
    return q[..., 0].astype(np.uint8)


def binarise(mask):
    with np.errstate(invalid="ignore"):
        return (np.asarray(mask, dtype=np.float32) >= np.float32(0.5)).astype(np.uint8)


def _footprints(a):
    h, w = a.shape[-2:]
    y0, x0 = 2 * np.arange((h + 1) // 2), 2 * np.arange((w + 1) // 2)
    y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
    a = a.astype(np.int64)
    return a[..., y0, :][..., x0], a[..., y0, :][..., x1], a[..., y1, :][..., x0], a[..., y1, :][..., x1]


def down_luma(a):
    p, q, r, s = _footprints(a)
    return ((p + q + r + s + 2) >> 2).astype(np.uint8)


def down_mask(m):
    p, q, r, s = _footprints(m)
    return (p | q | r | s).astype(np.uint8)


def pyramid(a, levels, down):
    out = [np.asarray(a, dtype=np.uint8)]
    for _ in range(levels - 1):
        out.append(down(out[-1]))
    return out


def grid_of(h, w):
    return (h + BLOCK - 1) // BLOCK, (w + BLOCK - 1) // BLOCK


def match_level(Ys, Yt, m, parent, search, smooth, subpel):
    """One level of one step: (vec int64 [gh, gw, 2] in 1/16 px as (vy, vx), valid bool [gh, gw]).  `parent` is the level above's
    final field or None at the coarsest level; `subpel` is True at level 0 only.  An invalid block holds 16 p."""
    h, w = Ys.shape
    gh, gw = grid_of(h, w)
    R, n = search, 2 * search + 1
    Ys, Yt, m = Ys.astype(np.int64), Yt.astype(np.int64), m.astype(np.int64)
    vec, valid = np.zeros((gh, gw, 2), np.int64), np.zeros((gh, gw), bool)
    for by in range(gh):
        for bx in range(gw):
            py = px = 0
            if parent is not None:
                pv = parent[min(by >> 1, parent.shape[0] - 1), min(bx >> 1, parent.shape[1] - 1)]
                py, px = 2 * ((int(pv[0]) + 8) >> 4), 2 * ((int(pv[1]) + 8) >> 4)
            y0, y1 = max(by * BLOCK - HALO, 0), min(by * BLOCK + BLOCK + HALO, h)
            x0, x1 = max(bx * BLOCK - HALO, 0), min(bx * BLOCK + BLOCK + HALO, w)
            mm = m[y0:y1, x0:x1]
            vec[by, bx] = (16 * py, 16 * px)
            if mm.sum() < MIN_PIXELS:
                continue
            valid[by, bx] = True
            win, ys, xs = Ys[y0:y1, x0:x1], np.arange(y0, y1), np.arange(x0, x1)
            S = np.zeros((n, n), np.int64)
            best = None
            for oy in range(-R, R + 1):
                ty = np.clip(ys + py + oy, 0, h - 1)
                for ox in range(-R, R + 1):
                    tx = np.clip(xs + px + ox, 0, w - 1)
                    s = int((np.abs(win - Yt[ty][:, tx]) * mm).sum())
                    S[oy + R, ox + R] = s
                    dist, idx = abs(oy) + abs(ox), (oy + R) * n + ox + R
                    key = ((s + smooth * dist) << 12) | (dist << 8) | idx
                    if best is None or key < best[0]:
                        best = (key, oy, ox)
            _, oy, ox = best
            v = [16 * (py + oy), 16 * (px + ox)]
            s0 = int(S[oy + R, ox + R])
            if subpel and s0 != 0:
                for axis, o in ((0, oy), (1, ox)):
                    if abs(o) == R:
                        continue
                    cm = int(S[oy + R - 1, ox + R] if axis == 0 else S[oy + R, ox + R - 1])
                    cp = int(S[oy + R + 1, ox + R] if axis == 0 else S[oy + R, ox + R + 1])
                    d = cm + cp - 2 * s0
                    if d > 0:
                        g = cm - cp
                        v[axis] += (1 if g > 0 else -1 if g < 0 else 0) * min(abs(8 * g) // d, 8)
            vec[by, bx] = v
    return vec, valid


def fill(vec, valid):
    """LP_PROP_FILL_ITERS Jacobi passes: an invalid block takes floor((2 sum + n) / (2 n)) over its n valid 3 x 3 neighbours."""
    vec, valid = vec.astype(np.int64).copy(), valid.copy()
    gh, gw = valid.shape
    for _ in range(FILL_ITERS):
        nv, nok = vec.copy(), valid.copy()
        for by in range(gh):
            for bx in range(gw):
                if valid[by, bx]:
                    continue
                ys, xs = slice(max(by - 1, 0), min(by + 2, gh)), slice(max(bx - 1, 0), min(bx + 2, gw))
                ok = valid[ys, xs]
                n = int(ok.sum())
                if n:
                    s = vec[ys, xs][ok].sum(axis=0)
                    nv[by, bx] = (2 * s + n) // (2 * n)               # Python's // is the floor
                    nok[by, bx] = True
        vec, valid = nv, nok
    return vec


def median3(vec):
    gh, gw = vec.shape[:2]
    p = np.pad(vec, ((1, 1), (1, 1), (0, 0)), mode="edge")
    stack = np.stack([p[dy:dy + gh, dx:dx + gw] for dy in range(3) for dx in range(3)])
    return np.sort(stack, axis=0)[4]


def fill_median(vec, valid):
    return median3(fill(vec, valid))


def motion_field(pyr_s, pyr_t, mpyr, search, smooth):
    """The final level-0 block field of one step, and every level's (raw vec, valid, final vec) for the stage tests."""
    L = len(pyr_s)
    parent, trace = None, [None] * L
    for lv in range(L - 1, -1, -1):
        raw, valid = match_level(pyr_s[lv], pyr_t[lv], mpyr[lv], parent, search, smooth, lv == 0)
        parent = fill_median(raw, valid)
        trace[lv] = (raw, valid, parent)
    return parent, trace


def pixel_vectors(vec, H, W):
    """Block field [gh, gw, 2] -> per-pixel [H, W, 2], bilinear between block centres in 1/16 weights."""
    gh, gw = vec.shape[:2]

    def axis(n, g):
        u = 2 * np.arange(n) - 7
        b0 = u >> 4
        return np.clip(b0, 0, g - 1), np.clip(b0 + 1, 0, g - 1), u - 16 * b0
    y0, y1, fy = axis(H, gh)
    x0, x1, fx = axis(W, gw)
    fy, fx = fy[:, None, None], fx[None, :, None]
    v = vec.astype(np.int64)
    top = (16 - fx) * v[y0][:, x0] + fx * v[y0][:, x1]
    bot = (16 - fx) * v[y1][:, x0] + fx * v[y1][:, x1]
    return ((16 - fy) * top + fy * bot + 128) >> 8


def bil(A, qy, qx):
    """The 256-weighted bilinear sample of A [H, W] or [H, W, K] at (qy, qx) in 1/16 px, clamped to the plane."""
    H, W = A.shape[:2]
    qy, qx = np.clip(qy, 0, 16 * (H - 1)), np.clip(qx, 0, 16 * (W - 1))
    iy, ix, fy, fx = qy >> 4, qx >> 4, qy & 15, qx & 15
    iy1, ix1 = np.minimum(iy + 1, H - 1), np.minimum(ix + 1, W - 1)
    A = A.astype(np.int64)
    if A.ndim == 3:
        fy, fx = fy[..., None], fx[..., None]
    return (16 - fy) * ((16 - fx) * A[iy, ix] + fx * A[iy, ix1]) + fy * ((16 - fx) * A[iy1, ix] + fx * A[iy1, ix1])


def key_positions(H, W):
    yy, xx = np.mgrid[:H, :W]
    return np.stack([16 * yy, 16 * xx], axis=-1).astype(np.int64)


def advance(P_s, vec, key_bits):
    """(P_t int64 [H, W, 2], c_t int64 [H, W] in 0..256) from the positions of s, the step's final level-0 field and the key bits."""
    H, W = key_bits.shape
    V = pixel_vectors(vec, H, W)
    yy, xx = np.mgrid[:H, :W]
    P_t = (bil(P_s, 16 * yy - V[..., 0], 16 * xx - V[..., 1]) + 128) >> 8
    return P_t, bil(key_bits, P_t[..., 0], P_t[..., 1])


def propagate_ref(images, mask, key_frame=0, levels=4, search=2, smooth=8, trace=None):
    """The whole chain: fp32 [F, H, W].  `trace`, a dict, receives per target frame (trace, P_t, c_t)."""
    images = np.asarray(images, dtype=np.float32)
    F, H, W = images.shape[:3]
    mask = np.asarray(mask, dtype=np.float32)
    if mask.ndim == 3:
        mask = mask[key_frame if mask.shape[0] == F and F > 1 else 0]
    key = binarise(mask)
    Y = luma(images)
    pyr = [pyramid(Y[f], levels, down_luma) for f in range(F)]
    out = np.zeros((F, H, W), np.float32)
    out[key_frame] = key
    for direction in (1, -1):
        P, bits = key_positions(H, W), key
        s = key_frame
        while 0 <= s + direction < F:
            t = s + direction
            vec, tr = motion_field(pyr[s], pyr[t], pyramid(bits, levels, down_mask), search, smooth)
            P, c = advance(P, vec, key)
            out[t] = (c.astype(np.float32) / np.float32(256))
            bits = (c >= 128).astype(np.uint8)
            if trace is not None:
                trace[t] = (tr, P, c)
            s = t
    return out
