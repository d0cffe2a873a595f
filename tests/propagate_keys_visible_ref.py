"""numpy restatement of the occlusion-aware video mask propagate from several keyframes, written from include/lanpaint_hip.h (the
section of lp_prop_visible_batch, lp_prop_occlude_batch and lp_prop_merge_visible).  The chain's stages are
tests/propagate_ref.py's, the occlusion test tests/propagate_visible_ref.py's, the plan of the chains and the merge's arithmetic
tests/propagate_keys_ref.py's; only the lost chains and the split of the merged code are added here.  Nothing here looks at the
kernels or at lanpaint_amd.propagate_keys_visible."""
import numpy as np

from tests import propagate_keys_ref as kref
from tests import propagate_ref as ref
from tests import propagate_visible_ref as vref
from tests import stabilize_ref as stab


def run_chain(pyr, key_bits, k, d, length, levels, search, smooth, occlusion):
    """`length` steps of the occlusion-aware chain from key frame k in direction d.  ({frame: (c, c', flags)} with c and c' int64
    [H, W] in 0..256 and flags int64 [gh, gw], and the counts N by step: [0] the key's bits, [s] the pixels with c' >= 128)."""
    H, W = key_bits.shape
    P, bits, out, counts = ref.key_positions(H, W), key_bits, {}, [int(key_bits.sum())]
    for s in range(1, length + 1):
        a, b = k + d * (s - 1), k + d * s
        vec, _ = ref.motion_field(pyr[a], pyr[b], ref.pyramid(bits, levels, ref.down_mask), search, smooth)
        P, c = ref.advance(P, vec, key_bits)
        flags = vref.visible_flags(pyr[b][0], pyr[k][0], P, (c >= 128).astype(np.uint8), occlusion)
        cv = vref.occlude(c, flags)
        out[b] = (c, cv, flags)
        bits = (cv >= 128).astype(np.uint8)
        counts.append(int(bits.sum()))
    return out, counts


def lost_at(counts, s):
    """Whether a chain with the counts `counts` (by step, [0] the key's) is lost at its step s: sticky, and never for a key with
    fewer than MIN_PIXELS bits."""
    return counts[0] >= ref.MIN_PIXELS and any(n < ref.MIN_PIXELS for n in counts[1:s + 1])


def split(c, cv):
    """(mask, hidden) fp32 of a code and its visible part."""
    return cv.astype(np.float32) / np.float32(256), (c - cv).astype(np.float32) / np.float32(256)


def merged_code(qa, qb, n, j):
    """c_S = (int)(S * 256.0f + 0.5f) of the merge S of two planes of signed squared distances: int64 in 0..256."""
    S = kref.merge(qa, qb, n, j)
    return ((S * np.float32(256)).astype(np.float32) + np.float32(0.5)).astype(np.float32).astype(np.int64)


def merge_frame(qa, qb, A, B, lost_a, lost_b, n, j):
    """One in-between frame: q the signed squared distances of the subject bits, A and B the chains' (c, c', flags)."""
    if lost_a != lost_b:
        c, cv, _ = B if lost_a else A
        return split(c, cv)
    cs = merged_code(qa, qb, n, j)
    flags = A[2] if 2 * j <= n else B[2]
    return split(cs, vref.occlude(cs, flags))


def subject_q(c):
    return stab.signed_d2_frame((c >= 128).astype(np.float32))


def propagate_keys_visible_ref(images, masks, keys, levels=4, search=2, smooth=8, occlusion=16, trace=None):
    """The whole rule: (mask, hidden), fp32 [F, H, W] each.  `trace`, a dict, receives "chains": {(key index, direction): (frames,
    counts)} and "lost": {frame: (A lost, B lost)} for the in-between frames.  occlusion = 0: the several-keys rule and zeros."""
    images = np.asarray(images, dtype=np.float32)
    F, H, W = images.shape[:3]
    keys = list(keys)
    if occlusion == 0:
        return kref.propagate_keys_ref(images, masks, keys, levels, search, smooth), np.zeros((F, H, W), np.float32)
    bits = [ref.binarise(m) for m in kref.key_masks(masks, keys, F)]
    pyr = kref.luma_pyramids(images, levels)
    out, hidden = np.zeros((F, H, W), np.float32), np.zeros((F, H, W), np.float32)
    for i, k in enumerate(keys):
        out[k] = bits[i]
    done = {(i, d): run_chain(pyr, bits[i], k, d, length, levels, search, smooth, occlusion)
            for i, k, d, length in kref.chain_plan(F, keys)}
    lost = {}
    for (i, d), (frames, _) in done.items():
        if (d < 0 and i == 0) or (d > 0 and i == len(keys) - 1):      # outside [k_0, k_{K-1}]: the one chain, lost or not
            for t, (c, cv, _) in frames.items():
                out[t], hidden[t] = split(c, cv)
    for i in range(len(keys) - 1):
        a, b = keys[i], keys[i + 1]
        if b - a < 2:
            continue
        (fa, na), (fb, nb) = done[(i, 1)], done[(i + 1, -1)]
        for t in range(a + 1, b):
            lost[t] = (lost_at(na, t - a), lost_at(nb, b - t))
            out[t], hidden[t] = merge_frame(subject_q(fa[t][0]), subject_q(fb[t][0]), fa[t], fb[t], *lost[t], b - a, t - a)
    if trace is not None:
        trace["chains"], trace["lost"] = done, lost
    return out, hidden
