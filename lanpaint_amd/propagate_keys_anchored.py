"""Video mask propagate from several keyframes, anchored: every chain matches its key frame again on every frame, so the drift
that is left between two keys does not add up.

`propagate_keys.propagate_keys` pins the mask to each painting, but half way through a long gap both chains have fallen behind
the subject: each composes one-frame fields whose sub-pixel estimates are pulled towards zero, as propagate_anchored.py says of
the single-key chain.  Here every chain is the anchored chain of its key; the plan, the gaps and the merge are propagate_keys's.

propagate_keys_anchored(images, masks, key_frames, levels=4, search=2, smooth=8, anchor=2) -> mask [F, H, W]
        `images`, `masks` and `key_frames` as propagate_keys takes them.  Behind every advance of every chain: the key frame's
        luma, sampled through the positions the chain carries, is matched against the frame per 8 x 8 block, +-`anchor` pixels,
        no predictor, the chain's `smooth`; fill and median run on that field and a second advance carries the positions along
        it.  Its mask is the chain's output at that frame and gives the bits that weight the next step's match.  A key frame
        returns its binarised painting, a frame outside the keys its one chain's output, a frame between two keys the merge of
        propagate_keys.  One key gives `propagate_anchored.propagate_masks_anchored` bit for bit; anchor = 0 switches the
        correction off: propagate_keys, no further launch.  A still video with the same mask on every key returns that
        binarised mask; empty stays exactly 0, full exactly 1.  include/lanpaint_hip.h (the several-keys anchored section)
        states the rule.  Not handled: occlusion -- anchoring inside propagate_keys_visible needs a gated batch; a subject whose
        look changes away from its key; re-anchoring every n-th frame only.  (That gated batch is propagate_keys_anchored_visible.py's:
        several keys, anchored and occlusion-aware.)  profiles/r38_propagate_keys_anchored.md has the numbers.

HIP tensors only, no CPU fallback, no device -> host read.  The re-match of up to 32 chains is one launch, lp_prop_match_batch in
its warped-key form (`propagate_keys.anchor_field_batch` is that launch on its own); a step of a group is 2 levels + 4 launches
and allocates nothing.  Memory as propagate_keys, and per chain one more position map and one more mask pyramid.
"""
from __future__ import annotations

import torch

from . import propagate_keys, stabilize
from ._hostcall import int_in
from ._motion import MAX_SEARCH, check_params
from .propagate_keys import Chains, Gaps, anchor_field_batch, clip_pyramids, merge_gap, painted_keys     # noqa: F401

MAX_ANCHOR = MAX_SEARCH
DEFAULT_ANCHOR = 2


def propagate_keys_anchored(images, masks, key_frames, levels=4, search=2, smooth=8, anchor=DEFAULT_ANCHOR):
    """The masks painted on the frames `key_frames` of `images` [F, H, W, C], every chain re-matched against its key on every
    frame, merged between the keys (module docstring): fp32 [F, H, W] on the images' device.  No device -> host read."""
    check_params(levels, search, smooth)
    int_in(anchor, 0, MAX_ANCHOR, "anchor")
    if anchor == 0:
        return propagate_keys.propagate_keys(images, masks, key_frames, levels, search, smooth)
    plan, keys, key_pyrs, (out,) = painted_keys(images, masks, key_frames, levels, __name__)
    (F, H, W, _), dev = images.shape, images.device
    if not plan:
        return out
    # as propagate_keys: a gap's forward chain writes into `out`, its backward chain into `back`, the merge overwrites the gap
    gaps = Gaps(keys)
    back = torch.empty((gaps.between, H, W), dtype=torch.float32, device=dev)
    outs = [gaps.stacked(back, c) if c[2] < 0 and gaps.of(c) else gaps.in_place(out, c) for c in plan]
    chains = Chains(plan, clip_pyramids(images, levels), key_pyrs, outs, H, W, levels, search, smooth, rematch=(anchor,))
    for s in range(1, int(chains.length.max()) + 1):
        chains.step(s)
    for a, b in gaps.pairs:
        mid, r = out[a + 1:b], gaps.first[a, b]
        merge_gap(stabilize.signed_d2(mid), stabilize.signed_d2(back[r:r + b - a - 1]), b - a, 1, mid)
    return out
