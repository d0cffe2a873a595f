"""numpy restatement of the occlusion-aware video mask propagate, written from include/lanpaint_hip.h (lp_prop_visible,
lp_prop_occlude) on top of tests/propagate_ref.py's stages: the key frame's luma is sampled through the carried positions, a block
whose picture no longer looks like the key's is flagged, and the mask code is weighted by the interpolated flags.  All of it in
integers.  Nothing here looks at the kernels."""
import numpy as np

from tests import propagate_ref as ref

VIS_MAX_BIAS = 32


def warped_key_luma(Yk, P):
    """K = (bil(Yk, P_t) + 128) >> 8: what the key frame shows at the position every pixel of t came from, 0..255."""
    return (ref.bil(Yk, P[..., 0], P[..., 1]) + 128) >> 8


def visible_flags(Yt, Yk, P, m, occlusion):
    """One flag per level-0 block, int64 [gh, gw]: 1 where the mask pixels of the block's window differ from the warped key luma,
    after a bias of at most VIS_MAX_BIAS is forgiven, by more than `occlusion` grey levels in the mean."""
    H, W = Yt.shape
    d = Yt.astype(np.int64) - warped_key_luma(Yk, P)
    gh, gw = ref.grid_of(H, W)
    flags = np.zeros((gh, gw), np.int64)
    for by in range(gh):
        for bx in range(gw):
            ys = slice(max(by * ref.BLOCK - ref.HALO, 0), min(by * ref.BLOCK + ref.BLOCK + ref.HALO, H))
            xs = slice(max(bx * ref.BLOCK - ref.HALO, 0), min(bx * ref.BLOCK + ref.BLOCK + ref.HALO, W))
            dd = d[ys, xs][m[ys, xs] != 0]
            n = int(dd.size)
            if n < ref.MIN_PIXELS:
                continue
            D = int(dd.sum())
            mu = max(-VIS_MAX_BIAS, min(VIS_MAX_BIAS, (2 * D + n) // (2 * n)))        # Python's // is the floor
            flags[by, bx] = int(np.abs(dd - mu).sum()) > occlusion * n
    return flags


def visibility_weight(flags, H, W):
    """w in 0..256 per pixel: v = 1 - flag interpolated between block centres as the advance interpolates the field, unrounded."""
    gh, gw = flags.shape

    def axis(n, g):
        u = 2 * np.arange(n) - 7
        b0 = u >> 4
        return np.clip(b0, 0, g - 1), np.clip(b0 + 1, 0, g - 1), u - 16 * b0
    y0, y1, fy = axis(H, gh)
    x0, x1, fx = axis(W, gw)
    fy, fx = fy[:, None], fx[None, :]
    v = 1 - flags.astype(np.int64)
    return (16 - fy) * ((16 - fx) * v[y0][:, x0] + fx * v[y0][:, x1]) + fy * ((16 - fx) * v[y1][:, x0] + fx * v[y1][:, x1])


def occlude(c, flags):
    """The visible part c' of the mask code c (both int64 [H, W] in 0..256); c - c' is the hidden part."""
    return (c.astype(np.int64) * visibility_weight(flags, *c.shape) + 128) >> 8


def propagate_visible_ref(images, mask, key_frame=0, levels=4, search=2, smooth=8, occlusion=16, trace=None):
    """The whole chain: (mask fp32 [F, H, W], hidden fp32 [F, H, W]).  `trace`, a dict, receives per target frame
    (P_t, c_t, flags, c'_t).  occlusion = 0: the plain chain and zeros."""
    images = np.asarray(images, dtype=np.float32)
    F, H, W = images.shape[:3]
    if occlusion == 0:
        return ref.propagate_ref(images, mask, key_frame, levels, search, smooth), np.zeros((F, H, W), np.float32)
    mask = np.asarray(mask, dtype=np.float32)
    if mask.ndim == 3:
        mask = mask[key_frame if mask.shape[0] == F and F > 1 else 0]
    key = ref.binarise(mask)
    Y = ref.luma(images)
    pyr = [ref.pyramid(Y[f], levels, ref.down_luma) for f in range(F)]
    out, hidden = np.zeros((F, H, W), np.float32), np.zeros((F, H, W), np.float32)
    out[key_frame] = key
    for direction in (1, -1):
        P, bits = ref.key_positions(H, W), key
        s = key_frame
        while 0 <= s + direction < F:
            t = s + direction
            vec, _ = ref.motion_field(pyr[s], pyr[t], ref.pyramid(bits, levels, ref.down_mask), search, smooth)
            P, c = ref.advance(P, vec, key)
            flags = visible_flags(Y[t], Y[key_frame], P, (c >= 128).astype(np.uint8), occlusion)
            cv = occlude(c, flags)
            out[t] = cv.astype(np.float32) / np.float32(256)
            hidden[t] = (c - cv).astype(np.float32) / np.float32(256)
            bits = (cv >= 128).astype(np.uint8)
            if trace is not None:
                trace[t] = (P, c, flags, cv)
            s = t
    return out, hidden
