"""Video mask propagate, anchored: every frame is matched against the key frame again, so drift does not add up on long clips.

`propagate.propagate_masks` composes one-frame motion fields.  Every step's sub-pixel estimate is pulled towards zero by `smooth`
and by the parabola fit, and nothing ever looks at the key frame again: on a subject that moves a fraction of a pixel per frame the
mask falls behind, a little more with every frame.  The position map every step carries names, for each pixel of frame t, where it
was in the key frame; the key frame's luma sampled through it is the picture the chain believes frame t to be.  Matching that
picture against the real frame t measures the error the chain has built up, and one more advance along it takes the error out.

propagate_masks_anchored(images, mask, key_frame=0, levels=4, search=2, smooth=8, anchor=2) -> mask [F, H, W]
        The single-key chain with three launches behind every advance.  lp_prop_anchor_match: per 8 x 8 block the masked block
        match of the single-key rule at level 0, the warped key luma as its source, the frame as its target, no predictor,
        +-`anchor` pixels, the chain's `smooth`, the sub-pixel step; warp and match are one launch, the warped picture never goes
        to memory.  The existing fill and median run on that field and the existing advance carries the positions along it; its
        mask is the step's output and gives the bits that weight the next step's match.  Nothing is remembered between frames
        but the positions.  The key frame returns its binarised mask.  anchor = 0 switches the correction off: propagate_masks,
        no further launch.  Integer arithmetic throughout: a still video and a noise-free whole-pixel shift that the plain chain
        tracks exactly give a zero correction and the plain chain's bits; an empty mask gives 0, a full mask 1.0, one frame the
        binarised mask.  include/lanpaint_hip.h (lp_prop_anchor_match) states the rule in full.
        Not handled: anchoring inside the several-key occlusion-aware form (propagate_keys_visible.py) -- an occluded block would
        be matched against the occluder, and the batched re-match of propagate_keys_anchored.py, which anchors the several-key
        form, has no gate; a subject whose look changes away from the key frame (it turns, or the light changes beyond what `smooth`
        refuses) gets no correction there and drifts as before; re-anchoring every n-th frame only.  Anchoring inside the
        single-key occlusion-aware form, with a gate that keeps an occluded block out of the match: propagate_anchored_visible.py.
        The several-key occlusion-aware form is anchored by propagate_keys_anchored_visible.py, whose batched re-match has the gate.
        profiles/r36_propagate_anchored.md has the numbers.

HIP tensors only, no CPU fallback, no device -> host read.  The frames' luma pyramids come in propagate's chunks, under
propagate.WS_CAP_BYTES; the key frame's luma plane is copied once per chain, so it outlives its chunk.  A step is 2 levels + 4
launches and allocates nothing.
"""
from __future__ import annotations

import ctypes

import torch

from . import _cabi, propagate
from ._hostcall import int_in, launch, require_hip
from ._motion import check_frame_planes, check_images, check_params
from .propagate import Step                                          # noqa: F401  (the family's one step, options and all)

MAX_ANCHOR = propagate.MAX_SEARCH
DEFAULT_ANCHOR = 2


def anchor_field(pos, tgt, key, mask_bits, anchor=DEFAULT_ANCHOR, smooth=8, vec=None, valid=None):
    """The raw correction field of frame t: `pos` its positions int32 [H, W, 2], `tgt` and `key` level 0 of its and of the key
    frame's luma pyramid, `mask_bits` level 0 of the pyramid the advance wrote, all uint8 [H, W].  (vec int32 [gh, gw, 2],
    valid int32 [gh, gw]), what fill_median takes.  One launch."""
    int_in(anchor, 1, MAX_ANCHOR, "anchor")
    int_in(smooth, 0, propagate.MAX_SMOOTH, "smooth")
    H, W = check_frame_planes(pos, tgt, key, mask_bits, __name__)
    gh, gw = _cabi.prop_grid(H, W)
    vec = torch.empty((gh, gw, 2), dtype=torch.int32, device=tgt.device) if vec is None else vec
    valid = torch.empty((gh, gw), dtype=torch.int32, device=tgt.device) if valid is None else valid
    d = _cabi.LpPropAnchorDesc(H, W, anchor, smooth, pos.data_ptr(), tgt.data_ptr(), key.data_ptr(), mask_bits.data_ptr(),
                               vec.data_ptr(), valid.data_ptr())
    launch("lp_prop_anchor_match", tgt.device, ctypes.byref(d))
    return vec, valid


def propagate_masks_anchored(images, mask, key_frame=0, levels=4, search=2, smooth=8, anchor=DEFAULT_ANCHOR):
    """`mask`, painted on frame `key_frame` of `images` [F, H, W, C], followed through every frame and matched against the key
    frame again on each (module docstring): fp32 [F, H, W] on the images' device.  No device -> host read."""
    check_params(levels, search, smooth)
    int_in(anchor, 0, MAX_ANCHOR, "anchor")
    check_images(images)
    require_hip(mask, "mask", __name__)
    int_in(key_frame, 0, images.shape[0] - 1, "key_frame")
    if anchor == 0:
        return propagate.propagate_masks(images, mask, key_frame, levels, search, smooth)
    return propagate.run(images, mask, key_frame, levels, search, smooth, rematch=(anchor_field, anchor, smooth))
