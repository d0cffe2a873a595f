"""numpy restatement of the anchored video mask propagate from several keyframes, written from include/lanpaint_hip.h (the
several-keys anchored section): tests/propagate_keys_ref.py's rule -- its plan, its key frames, its merge -- with every chain the
anchored chain of its key, made of tests/propagate_ref.py's motion field and advance and tests/propagate_anchored_ref.py's
anchored step.  Nothing here looks at the kernels or at the package."""
import numpy as np

from tests import propagate_anchored_ref as aref
from tests import propagate_keys_ref as kref
from tests import propagate_ref as ref


def run_chain(pyr, Y, key_bits, k, d, length, levels, search, smooth, anchor):
    """`length` steps of the anchored chain from key frame k in direction d: {frame: fp32 [H, W]}.  `pyr` the frames' luma
    pyramids, `Y` their luma planes; the key frame of the chain is the frame every step is matched against again."""
    H, W = key_bits.shape
    P, bits, out = ref.key_positions(H, W), key_bits, {}
    for s in range(1, length + 1):
        a, b = k + d * (s - 1), k + d * s
        vec, _ = ref.motion_field(pyr[a], pyr[b], ref.pyramid(bits, levels, ref.down_mask), search, smooth)
        P1, c1 = ref.advance(P, vec, key_bits)
        P, c, _ = aref.anchored_step(P1, c1, Y[b], Y[k], key_bits, anchor, smooth)
        out[b] = c.astype(np.float32) / np.float32(256)
        bits = (c >= 128).astype(np.uint8)
    return out


def propagate_keys_anchored_ref(images, masks, keys, levels=4, search=2, smooth=8, anchor=2, parts=None):
    """The whole rule: fp32 [F, H, W].  anchor = 0: the several-keys rule."""
    images = np.asarray(images, dtype=np.float32)
    keys = list(keys)
    if anchor == 0:
        return kref.propagate_keys_ref(images, masks, keys, levels, search, smooth, parts=parts)
    Y = ref.luma(images)
    pyr = [ref.pyramid(Y[f], levels, ref.down_luma) for f in range(Y.shape[0])]
    bits = [ref.binarise(m) for m in kref.key_masks(masks, keys, images.shape[0])]
    chain = lambda i, k, d, length: run_chain(pyr, Y, bits[i], k, d, length, levels, search, smooth, anchor)    # noqa: E731
    return kref.propagate_keys_ref(images, masks, keys, levels, search, smooth, chain=chain, parts=parts)
