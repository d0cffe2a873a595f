"""Video mask propagate, anchored and occlusion-aware: every frame is matched against the key frame again, and the mask stays off
whatever passes in front of the subject.

The two single-key refinements each fail where the other works.  `propagate_visible` tests against the key frame through positions
that have drifted: on a subject that moves a fraction of a pixel per frame drift reads as occlusion, the bits that weight the next
match go and the chain collapses, with no occluder in the clip.  `propagate_anchored` pulls the blocks under an occluder onto the
occluder, and the mask stays there while the subject moves on behind it.  The rotoscoping case that matters -- a long clip, a
subject moving a fraction of a pixel per frame, something passing in front -- needs both at once.

propagate_masks_anchored_visible(images, mask, key_frame=0, levels=4, search=2, smooth=8, anchor=2, occlusion=16)
        -> (mask [F, H, W], hidden [F, H, W])
        The single-key chain with six launches behind every step's fields.  lp_prop_anchor_match_gated: the anchored form's
        re-match (the warped key luma against the frame, per 8 x 8 block under the mask, +-`anchor` pixels, the chain's `smooth`,
        the sub-pixel step) and, in the same pass, lp_prop_visible's statistic at the alignment the match found: a block whose mask
        pixels differ from the key by more than `occlusion` grey levels in the mean, a brightness bias of at most 32 forgiven,
        even where the match fits best is gated -- it is behind something, and gives no correction.  Drift of up to `anchor`
        pixels is therefore not taken for an occluder.  The existing fill gives a gated block the correction of its visible
        neighbours, the existing advance carries the positions along that field, and the existing lp_prop_visible and
        lp_prop_occlude run on the corrected positions: `mask`, `hidden` and the bits that weight the next step's match are
        theirs, as in the occlusion-aware form.  Nothing is remembered between frames but the positions.  The key frame returns
        its binarised mask and a zero `hidden`.  anchor = 0 is propagate_masks_visible, occlusion = 0 propagate_masks_anchored and
        zeros, both 0 propagate_masks and zeros, each with its own launches only.  Integer arithmetic throughout: a still video and
        a noise-free whole-pixel shift that the plain chain tracks exactly return the plain chain's bits and a zero `hidden`; an
        empty mask gives 0 and 0, one frame the binarised mask; where no block is gated and no flag fires, `mask` is the anchored
        form's, bit for bit.  include/lanpaint_hip.h (lp_prop_anchor_match_gated) states the rule in full.
        Not handled: a subject hidden entirely; what leaves the picture; occlusion edges finer than a block --
        `LanPaint_MaskRefine` follows in the chain; several keys; a subject whose look changes away from the key.
        (Several keys, every chain this one: propagate_keys_anchored_visible.py.)
        profiles/r37_propagate_anchored_visible.md has the numbers.

HIP tensors only, no CPU fallback, no device -> host read.  The frames' luma pyramids come in propagate's chunks, under
propagate.WS_CAP_BYTES; the key frame's luma plane is copied once per chain, so it outlives its chunk.  A step is 2 levels + 6
launches and allocates nothing.
"""
from __future__ import annotations

import ctypes

import torch

from . import _cabi, propagate
from ._hostcall import int_in, launch, require_hip
from ._motion import check_frame_planes, check_images, check_params
from .propagate import Step                                          # noqa: F401  (the family's one step, options and all)
from .propagate_anchored import DEFAULT_ANCHOR, MAX_ANCHOR, propagate_masks_anchored
from .propagate_visible import DEFAULT_OCCLUSION, MAX_OCCLUSION, occlude, propagate_masks_visible, visible_flags


def gated_anchor_field(pos, tgt, key, mask_bits, anchor=DEFAULT_ANCHOR, smooth=8, occlusion=DEFAULT_OCCLUSION, vec=None, valid=None,
                       gated=None):
    """propagate_anchored.anchor_field with the occlusion gate: (vec int32 [gh, gw, 2], valid int32 [gh, gw], what fill_median
    takes, and gated int32 [gh, gw], 1 where a live block does not look like the key at the alignment its match found; there
    vec and valid are 0).  One launch."""
    int_in(anchor, 1, MAX_ANCHOR, "anchor")
    int_in(smooth, 0, propagate.MAX_SMOOTH, "smooth")
    int_in(occlusion, 1, MAX_OCCLUSION, "occlusion")
    H, W = check_frame_planes(pos, tgt, key, mask_bits, __name__)
    gh, gw = _cabi.prop_grid(H, W)
    vec = torch.empty((gh, gw, 2), dtype=torch.int32, device=tgt.device) if vec is None else vec
    valid = torch.empty((gh, gw), dtype=torch.int32, device=tgt.device) if valid is None else valid
    gated = torch.empty((gh, gw), dtype=torch.int32, device=tgt.device) if gated is None else gated
    d = _cabi.LpPropAnchorGatedDesc(H, W, anchor, smooth, occlusion, 0, pos.data_ptr(), tgt.data_ptr(), key.data_ptr(),
                                    mask_bits.data_ptr(), vec.data_ptr(), valid.data_ptr(), gated.data_ptr())
    launch("lp_prop_anchor_match_gated", tgt.device, ctypes.byref(d))
    return vec, valid, gated


def propagate_masks_anchored_visible(images, mask, key_frame=0, levels=4, search=2, smooth=8, anchor=DEFAULT_ANCHOR,
                                     occlusion=DEFAULT_OCCLUSION):
    """`mask`, painted on frame `key_frame` of `images` [F, H, W, C], followed through every frame, matched against the key frame
    again on each and kept off what passes in front of it (module docstring): (mask, hidden), fp32 [F, H, W] each, on the images'
    device.  No device -> host read."""
    check_params(levels, search, smooth)
    int_in(anchor, 0, MAX_ANCHOR, "anchor")
    int_in(occlusion, 0, MAX_OCCLUSION, "occlusion")
    check_images(images)
    require_hip(mask, "mask", __name__)
    F, H, W, _ = images.shape
    int_in(key_frame, 0, F - 1, "key_frame")
    if anchor == 0:
        return propagate_masks_visible(images, mask, key_frame, levels, search, smooth, occlusion)
    if occlusion == 0:
        return (propagate_masks_anchored(images, mask, key_frame, levels, search, smooth, anchor),
                images.new_zeros((F, H, W), dtype=torch.float32))
    return propagate.run(images, mask, key_frame, levels, search, smooth, rematch=(gated_anchor_field, anchor, smooth, occlusion),
                         split=(visible_flags, occlude, occlusion))
