"""numpy restatement of the anchored video mask propagate, written from include/lanpaint_hip.h (lp_prop_anchor_match) on top of
tests/propagate_ref.py's stages: behind every advance the key frame's luma, sampled through the carried positions, is matched
against the real frame; the block field of that match is the error the chain has built up, and one more advance along it takes the
error out.  All of it in integers.  Nothing here looks at the kernels."""
import numpy as np

from tests import propagate_ref as ref


def warped_key_luma(Yk, P):
    """K = (bil(Yk, P_t) + 128) >> 8: what the key frame shows at the position every pixel of t came from, 0..255."""
    return ((ref.bil(Yk, P[..., 0], P[..., 1]) + 128) >> 8).astype(np.uint8)


def anchor_field(P, Yt, Yk, m, anchor, smooth):
    """The raw correction field of frame t: (vec int64 [gh, gw, 2] in 1/16 px, valid bool [gh, gw]).  The single-key match at
    level 0 with the warped key luma as the source, the frame as the target, predictor 0; an invalid block holds 0."""
    return ref.match_level(warped_key_luma(Yk, P), Yt, m, None, anchor, smooth, True)


def anchored_step(P, c, Yt, Yk, key_bits, anchor, smooth):
    """(P', c', e) from the first advance's (P_t, c): the match, fill and median, and the second advance along e."""
    raw, valid = anchor_field(P, Yt, Yk, (c >= 128).astype(np.uint8), anchor, smooth)
    e = ref.fill_median(raw, valid)
    P2, c2 = ref.advance(P, e, key_bits)
    return P2, c2, e


def propagate_anchored_ref(images, mask, key_frame=0, levels=4, search=2, smooth=8, anchor=2, trace=None):
    """The whole chain: fp32 [F, H, W].  `trace`, a dict, receives per target frame (P_t, c_t, e, P'_t, c'_t).  anchor = 0: the
    plain chain."""
    images = np.asarray(images, dtype=np.float32)
    if anchor == 0:
        return ref.propagate_ref(images, mask, key_frame, levels, search, smooth)
    F, H, W = images.shape[:3]
    mask = np.asarray(mask, dtype=np.float32)
    if mask.ndim == 3:
        mask = mask[key_frame if mask.shape[0] == F and F > 1 else 0]
    key = ref.binarise(mask)
    Y = ref.luma(images)
    pyr = [ref.pyramid(Y[f], levels, ref.down_luma) for f in range(F)]
    out = np.zeros((F, H, W), np.float32)
    out[key_frame] = key
    for direction in (1, -1):
        P, bits = ref.key_positions(H, W), key
        s = key_frame
        while 0 <= s + direction < F:
            t = s + direction
            vec, _ = ref.motion_field(pyr[s], pyr[t], ref.pyramid(bits, levels, ref.down_mask), search, smooth)
            P1, c1 = ref.advance(P, vec, key)
            P, c, e = anchored_step(P1, c1, Y[t], Y[key_frame], key, anchor, smooth)
            out[t] = c.astype(np.float32) / np.float32(256)
            bits = (c >= 128).astype(np.uint8)
            if trace is not None:
                trace[t] = (P1, c1, e, P, c)
            s = t
    return out
