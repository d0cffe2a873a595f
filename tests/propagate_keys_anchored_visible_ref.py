"""numpy restatement of the anchored occlusion-aware video mask propagate from several keyframes, written from
include/lanpaint_hip.h (the several-keys anchored and occlusion-aware section): the several-keys occlusion-aware rule -- its plan,
its key frames, its lost chains, its merge and split -- with every chain the anchored occlusion-aware chain of its own key.  The
pieces are the existing restatements': tests/propagate_ref.py's motion field, advance and fill, tests/propagate_anchored_visible_ref.py's
gated anchor field, tests/propagate_visible_ref.py's flags and occlude, tests/propagate_keys_visible_ref.py's lost rule and merge,
tests/propagate_keys_ref.py's plan and key masks.  Nothing here looks at the kernels or at the package."""
import numpy as np

from tests import propagate_anchored_visible_ref as avref
from tests import propagate_keys_anchored_ref as karef
from tests import propagate_keys_ref as kref
from tests import propagate_keys_visible_ref as kvref
from tests import propagate_ref as ref
from tests import propagate_visible_ref as vref


def run_chain(pyr, key_bits, k, d, length, levels, search, smooth, anchor, occlusion):
    """`length` steps of the anchored occlusion-aware chain from key frame k in direction d, every step matched against frame k
    again.  ({frame: (c, c', flags)} as tests/propagate_keys_visible_ref.py's run_chain gives them, and the counts N by step)."""
    H, W = key_bits.shape
    Yk = pyr[k][0]
    P, bits, out, counts = ref.key_positions(H, W), key_bits, {}, [int(key_bits.sum())]
    for s in range(1, length + 1):
        a, b = k + d * (s - 1), k + d * s
        vec, _ = ref.motion_field(pyr[a], pyr[b], ref.pyramid(bits, levels, ref.down_mask), search, smooth)
        P1, c1 = ref.advance(P, vec, key_bits)
        raw, valid, _ = avref.gated_anchor_field(P1, pyr[b][0], Yk, (c1 >= 128).astype(np.uint8), anchor, smooth, occlusion)
        P, c = ref.advance(P1, ref.fill_median(raw, valid), key_bits)
        flags = vref.visible_flags(pyr[b][0], Yk, P, (c >= 128).astype(np.uint8), occlusion)
        cv = vref.occlude(c, flags)
        out[b] = (c, cv, flags)
        bits = (cv >= 128).astype(np.uint8)
        counts.append(int(bits.sum()))
    return out, counts


def propagate_keys_anchored_visible_ref(images, masks, keys, levels=4, search=2, smooth=8, anchor=2, occlusion=16, trace=None,
                                        chain=None):
    """The whole rule: (mask, hidden), fp32 [F, H, W] each.  `trace`, a dict, receives "chains": {(key index, direction): (frames,
    counts)} and "lost": {frame: (A lost, B lost)} for the in-between frames.  anchor = 0: the several-keys occlusion-aware rule;
    occlusion = 0: the several-keys anchored rule and zeros; both 0: the several-keys rule and zeros.  `chain`, for a caller that
    has its chains already: (key index, key frame, direction, length) -> what run_chain returns for them."""
    images = np.asarray(images, dtype=np.float32)
    F, H, W = images.shape[:3]
    keys = list(keys)
    if anchor == 0:
        return kvref.propagate_keys_visible_ref(images, masks, keys, levels, search, smooth, occlusion, trace=trace)
    if occlusion == 0:
        return karef.propagate_keys_anchored_ref(images, masks, keys, levels, search, smooth, anchor), np.zeros((F, H, W), np.float32)
    bits = [ref.binarise(m) for m in kref.key_masks(masks, keys, F)]
    pyr = kref.luma_pyramids(images, levels)
    out, hidden = np.zeros((F, H, W), np.float32), np.zeros((F, H, W), np.float32)
    for i, k in enumerate(keys):
        out[k] = bits[i]
    if chain is None:
        chain = lambda i, k, d, length: run_chain(pyr, bits[i], k, d, length, levels, search, smooth, anchor, occlusion)    # noqa: E731
    done = {(i, d): chain(i, k, d, length) for i, k, d, length in kref.chain_plan(F, keys)}
    lost = {}
    for (i, d), (frames, _) in done.items():
        if (d < 0 and i == 0) or (d > 0 and i == len(keys) - 1):      # outside [k_0, k_{K-1}]: the one chain, lost or not
            for t, (c, cv, _) in frames.items():
                out[t], hidden[t] = kvref.split(c, cv)
    for i in range(len(keys) - 1):
        a, b = keys[i], keys[i + 1]
        if b - a < 2:
            continue
        (fa, na), (fb, nb) = done[(i, 1)], done[(i + 1, -1)]
        for t in range(a + 1, b):
            lost[t] = (kvref.lost_at(na, t - a), kvref.lost_at(nb, b - t))
            out[t], hidden[t] = kvref.merge_frame(kvref.subject_q(fa[t][0]), kvref.subject_q(fb[t][0]), fa[t], fb[t], *lost[t],
                                                  b - a, t - a)
    if trace is not None:
        trace["chains"], trace["lost"] = done, lost
    return out, hidden
