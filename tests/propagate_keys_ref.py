"""numpy restatement of the video mask propagate from several keyframes, written from include/lanpaint_hip.h (the lp_prop_*_batch
section).  The chain is tests/propagate_ref.py's and the signed squared distances and the capped root tests/stabilize_ref.py's;
only the plan of the chains and the merge are added here.  Nothing here looks at the kernels or at lanpaint_amd.propagate_keys."""
import numpy as np

from tests import propagate_ref as ref
from tests import stabilize_ref as stab


def chain_plan(frames, keys):
    """(key index, key frame, direction, length) in the rule's order; a chain of length 0 does not exist."""
    plan = [(0, keys[0], -1, keys[0])]
    for i in range(len(keys) - 1):
        n = keys[i + 1] - keys[i]
        plan.append((i, keys[i], 1, n - 1))
        plan.append((i + 1, keys[i + 1], -1, n - 1))
    plan.append((len(keys) - 1, keys[-1], 1, frames - 1 - keys[-1]))
    return [c for c in plan if c[3] >= 1]


def run_chain(pyr, key_bits, k, d, length, levels, search, smooth):
    """`length` steps of the chain from key frame k in direction d over the frames' luma pyramids `pyr`: {frame: fp32 [H, W]}.
    Step s goes from frame k + d (s - 1) to frame k + d s; a longer chain begins with the shorter one."""
    H, W = key_bits.shape
    P, bits, out = ref.key_positions(H, W), key_bits, {}
    for s in range(1, length + 1):
        a, b = k + d * (s - 1), k + d * s
        vec, _ = ref.motion_field(pyr[a], pyr[b], ref.pyramid(bits, levels, ref.down_mask), search, smooth)
        P, c = ref.advance(P, vec, key_bits)
        out[b] = c.astype(np.float32) / np.float32(256)
        bits = (c >= 128).astype(np.uint8)
    return out


def merge(qa, qb, n, j):
    """One frame of the merge: q int [H, W] signed squared distances, n the gap, j the frame's distance from the left key."""
    sa, sb = stab.capped_distance(np.asarray(qa, np.int64)), stab.capped_distance(np.asarray(qb, np.int64))
    pa = np.float64(n - j) * sa
    pb = np.float64(j) * sb
    acc = pa + pb
    sd = acc / np.float64(n)
    v = np.float64(0.5) + sd
    return np.minimum(np.maximum(v, 0.0), 1.0).astype(np.float32)


def merge_masks(A, B, n, j):
    return merge(stab.signed_d2_frame(A), stab.signed_d2_frame(B), n, j)


def luma_pyramids(images, levels):
    Y = ref.luma(np.asarray(images, dtype=np.float32))
    return [ref.pyramid(Y[f], levels, ref.down_luma) for f in range(Y.shape[0])]


def key_masks(masks, keys, F):
    masks = np.asarray(masks, dtype=np.float32)
    if masks.ndim == 2:
        masks = masks[None]
    return [masks[i] for i in (range(len(keys)) if masks.shape[0] == len(keys) else keys)]


def propagate_keys_ref(images, masks, keys, levels=4, search=2, smooth=8, chain=None, parts=None):
    """The whole rule: fp32 [F, H, W].  `chain(key index, k, d, length)` may supply a chain's frames (a cache); `parts`, a dict,
    receives per in-between frame (A, B)."""
    images = np.asarray(images, dtype=np.float32)
    F, H, W = images.shape[:3]
    keys = list(keys)
    bits = [ref.binarise(m) for m in key_masks(masks, keys, F)]
    if chain is None:
        pyr = luma_pyramids(images, levels)
        chain = lambda i, k, d, length: run_chain(pyr, bits[i], k, d, length, levels, search, smooth)    # noqa: E731
    out = np.zeros((F, H, W), np.float32)
    for i, k in enumerate(keys):
        out[k] = bits[i]
    done = {(i, d): chain(i, k, d, length) for i, k, d, length in chain_plan(F, keys)}
    for (i, d), frames in done.items():
        if (d < 0 and i == 0) or (d > 0 and i == len(keys) - 1):      # outside [k_0, k_{K-1}]: the one chain's output
            for t, m in frames.items():
                out[t] = m
    for i in range(len(keys) - 1):
        a, b = keys[i], keys[i + 1]
        for t in range(a + 1, b):
            A, B = done[(i, 1)][t], done[(i + 1, -1)][t]
            out[t] = merge_masks(A, B, b - a, t - a)
            if parts is not None:
                parts[t] = (A, B)
    return out
