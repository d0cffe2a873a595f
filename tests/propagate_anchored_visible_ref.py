"""numpy restatement of the anchored occlusion-aware video mask propagate, written from include/lanpaint_hip.h
(lp_prop_anchor_match_gated) on top of tests/propagate_ref.py, tests/propagate_anchored_ref.py and tests/propagate_visible_ref.py:
the anchored re-match, in which a block whose mask pixels do not look like the key frame at the alignment the match found gives
no correction, and the visible form's test and split on the corrected positions.  All of it in integers.  Nothing here looks at
the kernels."""
import numpy as np

from tests import propagate_anchored_ref as anc
from tests import propagate_ref as ref
from tests import propagate_visible_ref as vis


def whole_pixel_winners(K, Yt, m, anchor, smooth):
    """The candidate the key order chooses before the sub-pixel step, per level-0 block: (int64 [gh, gw, 2] as (oy, ox), live
    bool [gh, gw]).  The window, validity, candidates, key and clamping of ref.match_level at level 0 with predictor 0."""
    h, w = K.shape
    gh, gw = ref.grid_of(h, w)
    R, n = anchor, 2 * anchor + 1
    K, Yt, m = K.astype(np.int64), Yt.astype(np.int64), m.astype(np.int64)
    win, live = np.zeros((gh, gw, 2), np.int64), np.zeros((gh, gw), bool)
    for by in range(gh):
        for bx in range(gw):
            y0, y1 = max(by * ref.BLOCK - ref.HALO, 0), min(by * ref.BLOCK + ref.BLOCK + ref.HALO, h)
            x0, x1 = max(bx * ref.BLOCK - ref.HALO, 0), min(bx * ref.BLOCK + ref.BLOCK + ref.HALO, w)
            mm = m[y0:y1, x0:x1]
            if mm.sum() < ref.MIN_PIXELS:
                continue
            live[by, bx] = True
            src, ys, xs = K[y0:y1, x0:x1], np.arange(y0, y1), np.arange(x0, x1)
            best = None
            for oy in range(-R, R + 1):
                ty = np.clip(ys + oy, 0, h - 1)
                for ox in range(-R, R + 1):
                    tx = np.clip(xs + ox, 0, w - 1)
                    s = int((np.abs(src - Yt[ty][:, tx]) * mm).sum())
                    dist = abs(oy) + abs(ox)
                    key = ((s + smooth * dist) << 12) | (dist << 8) | ((oy + R) * n + ox + R)
                    if best is None or key < best[0]:
                        best = (key, oy, ox)
            win[by, bx] = best[1:]
    return win, live


def gate(K, Yt, m, win, live, occlusion):
    """int64 [gh, gw], 1 where a live block's mask pixels differ from K at the winner's alignment, after a bias of at most
    vis.VIS_MAX_BIAS is forgiven, by more than `occlusion` grey levels in the mean: lp_prop_visible's statistic, moved by (oy, ox)."""
    h, w = K.shape
    gh, gw = live.shape
    K, Yt = K.astype(np.int64), Yt.astype(np.int64)
    gated = np.zeros((gh, gw), np.int64)
    for by in range(gh):
        for bx in range(gw):
            if not live[by, bx]:
                continue
            y0, y1 = max(by * ref.BLOCK - ref.HALO, 0), min(by * ref.BLOCK + ref.BLOCK + ref.HALO, h)
            x0, x1 = max(bx * ref.BLOCK - ref.HALO, 0), min(bx * ref.BLOCK + ref.BLOCK + ref.HALO, w)
            oy, ox = (int(v) for v in win[by, bx])
            ty, tx = np.clip(np.arange(y0, y1) + oy, 0, h - 1), np.clip(np.arange(x0, x1) + ox, 0, w - 1)
            dd = (Yt[ty][:, tx] - K[y0:y1, x0:x1])[m[y0:y1, x0:x1] != 0]
            n = int(dd.size)
            D = int(dd.sum())
            mu = max(-vis.VIS_MAX_BIAS, min(vis.VIS_MAX_BIAS, (2 * D + n) // (2 * n)))        # Python's // is the floor
            gated[by, bx] = int(np.abs(dd - mu).sum()) > occlusion * n
    return gated


def gated_anchor_field(P, Yt, Yk, m, anchor, smooth, occlusion):
    """(vec int64 [gh, gw, 2], valid bool [gh, gw], gated int64 [gh, gw]): the anchored form's raw correction field where the
    block is not gated, 0 and not valid where it is."""
    K = anc.warped_key_luma(Yk, P)
    vec, valid = ref.match_level(K, Yt, m, None, anchor, smooth, True)
    win, live = whole_pixel_winners(K, Yt, m, anchor, smooth)
    assert (live == valid).all()
    gated = gate(K, Yt, m, win, live, occlusion)
    vec = np.where(gated[..., None] != 0, 0, vec)
    return vec, valid & (gated == 0), gated


def propagate_anchored_visible_ref(images, mask, key_frame=0, levels=4, search=2, smooth=8, anchor=2, occlusion=16, trace=None,
                                   gate_on=True):
    """The whole chain: (mask fp32 [F, H, W], hidden fp32 [F, H, W]).  `trace`, a dict, receives per target frame
    (P_t, c_t, gated, e, P'_t, c'_t, flags, the visible part of c'_t).  anchor = 0: the visible chain; occlusion = 0: the anchored
    chain and zeros.  gate_on = False leaves every live block its correction: the rule without its gate, for measurements."""
    images = np.asarray(images, dtype=np.float32)
    F, H, W = images.shape[:3]
    if anchor == 0:
        return vis.propagate_visible_ref(images, mask, key_frame, levels, search, smooth, occlusion)
    if occlusion == 0:
        return anc.propagate_anchored_ref(images, mask, key_frame, levels, search, smooth, anchor), np.zeros((F, H, W), np.float32)
    mask = np.asarray(mask, dtype=np.float32)
    if mask.ndim == 3:
        mask = mask[key_frame if mask.shape[0] == F and F > 1 else 0]
    key = ref.binarise(mask)
    Y = ref.luma(images)
    Yk = Y[key_frame]
    pyr = [ref.pyramid(Y[f], levels, ref.down_luma) for f in range(F)]
    out, hidden = np.zeros((F, H, W), np.float32), np.zeros((F, H, W), np.float32)
    out[key_frame] = key
    for direction in (1, -1):
        P, bits = ref.key_positions(H, W), key
        s = key_frame
        while 0 <= s + direction < F:
            t = s + direction
            vec, _ = ref.motion_field(pyr[s], pyr[t], ref.pyramid(bits, levels, ref.down_mask), search, smooth)
            P1, c1 = ref.advance(P, vec, key)
            m1 = (c1 >= 128).astype(np.uint8)
            if gate_on:
                raw, valid, gated = gated_anchor_field(P1, Y[t], Yk, m1, anchor, smooth, occlusion)
            else:
                raw, valid = anc.anchor_field(P1, Y[t], Yk, m1, anchor, smooth)
                gated = np.zeros(valid.shape, np.int64)
            e = ref.fill_median(raw, valid)
            P, c = ref.advance(P1, e, key)
            flags = vis.visible_flags(Y[t], Yk, P, (c >= 128).astype(np.uint8), occlusion)
            cv = vis.occlude(c, flags)
            out[t] = cv.astype(np.float32) / np.float32(256)
            hidden[t] = (c - cv).astype(np.float32) / np.float32(256)
            bits = (cv >= 128).astype(np.uint8)
            if trace is not None:
                trace[t] = (P1, c1, gated, e, P, c, flags, cv)
            s = t
    return out, hidden
