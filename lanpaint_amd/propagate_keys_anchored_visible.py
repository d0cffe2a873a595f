"""Video mask propagate from several keyframes, anchored and occlusion-aware: every painted key follows the picture's motion in both
directions, matches its key frame again on every frame and stays off what passes in front of the subject; between two keys a chain
that lost the subject gives way to the other.

This is the rotoscoping case that matters with the remedy a user reaches for: a long clip, a subject that moves a fraction of a
pixel per frame, something passing in front, and a second key painted behind the occluder.  `propagate_keys_visible` takes the
drift of such a clip for occlusion and its chains collapse; `propagate_keys_anchored` pulls the blocks under the occluder onto it
and has no `hidden`.  Here every chain is the anchored occlusion-aware chain of its key (propagate_anchored_visible.py's); the
plan, the lost chains and the merge are propagate_keys_visible's.

propagate_keys_anchored_visible(images, masks, key_frames, levels=4, search=2, smooth=8, anchor=2, occlusion=16)
        -> (mask [F, H, W], hidden [F, H, W])
        `images`, `masks` and `key_frames` as `propagate_keys` takes them, `anchor` as `propagate_keys_anchored`, `occlusion` as
        `propagate_keys_visible`.  Behind every advance of every chain: the key frame's luma, sampled through the positions the
        chain carries, is matched against the frame per 8 x 8 block, +-`anchor` pixels, and a block whose mask pixels do not look
        like the key at the alignment found, by more than `occlusion` grey levels in the mean, gives no correction (the gate);
        fill and median run on that field, a second advance carries the positions along it, and the occlusion test and the split
        into `mask` and `hidden` run on the corrected positions.  A key frame returns its binarised painting and a zero `hidden`;
        a frame outside the keys its one chain's (mask, hidden), which is `propagate_masks_anchored_visible` from the nearest key;
        a frame between two keys what `propagate_keys_visible` says of its chains: with exactly one chain lost the other chain's
        frame, otherwise the merge of the subjects split by the flags of the chain from the nearer key.  One key gives
        `propagate_masks_anchored_visible` bit for bit, both outputs.  anchor = 0 gives `propagate_keys_visible`, occlusion = 0
        `propagate_keys_anchored` and zeros, both 0 `propagate_keys` and zeros, each with its own launches only.  A still video
        with the same mask on every key returns that binarised mask and a zero `hidden`; empty keys everywhere give 0 and 0;
        mask + hidden is a multiple of 1/256.  include/lanpaint_hip.h (the several-keys anchored and occlusion-aware section)
        states the rule.  Not handled: following a subject through a full occlusion (the second key is what recovers it); what
        leaves the picture; occlusion edges finer than a block; a subject whose look changes away from its key.  Lost chains are
        not stopped early.  profiles/r39_propagate_keys_anchored_visible.md has the numbers.

HIP tensors only, no CPU fallback, no device -> host read.  The gated re-match of up to 32 chains is one launch, lp_prop_match_batch
in its gated form (`propagate_keys.anchor_field_batch` with `occlusion` is that launch on its own); a step of a group is
2 levels + 6 launches and allocates nothing.  Memory as propagate_keys_visible, and per chain one more position map; all of it
must fit WS_CAP_BYTES.
"""
from __future__ import annotations

import torch

from . import propagate_keys_anchored, propagate_keys_visible
from ._hostcall import int_in
from ._motion import check_params
from .propagate_keys import anchor_field_batch, chain_plan                                   # noqa: F401  (the node's, the tests')
from .propagate_keys_anchored import DEFAULT_ANCHOR, MAX_ANCHOR
from .propagate_keys_visible import DEFAULT_OCCLUSION, MAX_OCCLUSION, visible_chains

WS_CAP_BYTES = 1 << 30


def propagate_keys_anchored_visible(images, masks, key_frames, levels=4, search=2, smooth=8, anchor=DEFAULT_ANCHOR,
                                    occlusion=DEFAULT_OCCLUSION):
    """The masks painted on the frames `key_frames` of `images` [F, H, W, C], every chain re-matched against its key on every
    frame and kept off what passes in front, merged between the keys (module docstring): (mask, hidden), fp32 [F, H, W] each, on
    the images' device.  No device -> host read."""
    check_params(levels, search, smooth)
    int_in(anchor, 0, MAX_ANCHOR, "anchor")
    int_in(occlusion, 0, MAX_OCCLUSION, "occlusion")
    if anchor == 0:                                                  # an "off" route makes every further check itself
        return propagate_keys_visible.propagate_keys_visible(images, masks, key_frames, levels, search, smooth, occlusion)
    if occlusion == 0:
        out = propagate_keys_anchored.propagate_keys_anchored(images, masks, key_frames, levels, search, smooth, anchor)
        return out, torch.zeros_like(out)
    return visible_chains(images, masks, key_frames, levels, search, smooth, occlusion, __name__, WS_CAP_BYTES, anchor)
