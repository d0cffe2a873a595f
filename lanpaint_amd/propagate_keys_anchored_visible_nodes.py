"""LanPaint_VideoMaskPropagateKeysAnchoredVisible: masks painted on several frames follow the picture's motion, each matched against
its own key frame again on every frame, stay off whatever passes in front of the subject, and are merged between the keys so that a
chain that lost the subject gives way to the other.

LanPaint_VideoMaskPropagateKeysVisible takes the drift of a long clip whose subject moves a fraction of a pixel per frame for an
occluder; LanPaint_VideoMaskPropagateKeysAnchored takes the drift out and puts the mask onto whatever passes in front.  This node
(lanpaint_amd.propagate_keys_anchored_visible, on the HIP device) gives every chain LanPaint_VideoMaskPropagateAnchoredVisible's
step and joins the chains as the keys-visible node does: paint a second key behind the occluder.  It sits where the keys node sits:

    painted masks + the video -> VideoMaskPropagateKeysAnchoredVisible -> VideoMaskStabilize -> MaskRefine -> ImageEncode / DetailerCrop*

Occlusion edges are as coarse as the 8 x 8 blocks, which the mask refine sharpens; a subject is not followed through a full
occlusion, the next key recovers it; what leaves the picture is lost; where the subject stops looking like its key frame it counts
as covered.  Host tensors in and out like the other nodes.  The reference has no such node.
LanPaint_VideoMaskPropagateKeysAnchoredVisibleShots takes the `shots` of LanPaint_VideoShots and runs every shot on the keys that
lie inside it; with anchor and / or occlusion 0 it is the per-shot form of the other several-keys nodes.

This module has its own NODE_CLASS_MAPPINGS: merge them with the others' (INTEGRATION.md section 2(b)).
"""
from __future__ import annotations

from . import propagate_keys_anchored_visible as _both
from . import shots as _shots
from ._hostcall import int_in, node_device
from .propagate_anchored_visible_nodes import LanPaint_VideoMaskPropagateAnchoredVisible
from .propagate_keys_anchored_nodes import LanPaint_VideoMaskPropagateKeysAnchored
from .propagate_keys_nodes import LanPaint_VideoMaskPropagateKeys, parse_key_frames
from .shots_nodes import _PerShot


class LanPaint_VideoMaskPropagateKeysAnchoredVisible:
    """Carry masks painted on several frames through the video along the picture's motion, each re-matched against its key frame,
    keep them off what passes in front, and merge them between the keys."""

    @classmethod
    def INPUT_TYPES(s):
        required = dict(LanPaint_VideoMaskPropagateKeys.INPUT_TYPES()["required"])
        required["anchor"] = LanPaint_VideoMaskPropagateKeysAnchored.INPUT_TYPES()["required"]["anchor"]
        required["occlusion"] = LanPaint_VideoMaskPropagateAnchoredVisible.INPUT_TYPES()["required"]["occlusion"]
        return {"required": required}

    RETURN_TYPES = ("MASK", "MASK")
    RETURN_NAMES = ("mask", "hidden")
    OUTPUT_TOOLTIPS = ("The carried and merged mask without the part that something covers: what the sampler should repaint.",
                       "The part of the subject that is behind something, frame by frame. Add it back to the mask when you want "
                       "to inpaint through the occluder; leave it out to keep the occluder as it is.")
    FUNCTION = "propagate"
    CATEGORY = "mask"
    DESCRIPTION = ("Makes a per-frame video mask from masks painted on several key frames, like the video mask propagate from "
                   "keys: every key follows the picture's motion in both directions. Every frame is matched against its key frame "
                   "again, so the mask does not fall behind its subject half way through a long gap, and the mask is kept off "
                   "whatever passes in front of the subject: the covered part moves from `mask` to `hidden`. A block that is "
                   "covered takes no part in the re-match. When the subject is covered entirely, paint a second key behind the "
                   "occluder: between the two keys a chain that lost the subject gives way to the other, otherwise the two are "
                   "merged. The result equals the painting on every key. Put it in front of the video mask stabilize, the mask "
                   "refine, the encode and the Detailer crops. An empty key means nothing is there. Not handled: a subject "
                   "followed through a full occlusion without a second key, what leaves the picture, occlusion edges finer than a "
                   "block, and a subject whose look changes away from its key frame.")

    def _checked(self, image, key_frames, anchor, occlusion):
        """The keys, with every number refused before a device is looked for."""
        keys = parse_key_frames(key_frames)
        _both.chain_plan(int(image.shape[0]), keys)
        int_in(int(anchor), 0, _both.MAX_ANCHOR, "anchor")
        int_in(int(occlusion), 0, _both.MAX_OCCLUSION, "occlusion")
        return keys

    def propagate(self, image, mask, key_frames="0", levels=4, search=2, smooth=8, anchor=_both.DEFAULT_ANCHOR,
                  occlusion=_both.DEFAULT_OCCLUSION):
        keys = self._checked(image, key_frames, anchor, occlusion)
        dev = node_device(image)
        out, hidden = _both.propagate_keys_anchored_visible(image.to(dev), mask.to(dev), keys, int(levels), int(search), int(smooth),
                                                            int(anchor), int(occlusion))
        return (out.to(mask.device), hidden.to(mask.device))


class LanPaint_VideoMaskPropagateKeysAnchoredVisibleShots(_PerShot, LanPaint_VideoMaskPropagateKeysAnchoredVisible):
    DESCRIPTION = (LanPaint_VideoMaskPropagateKeysAnchoredVisible.DESCRIPTION + " With `shots` every shot is run on the keys that "
                   "lie inside it, and both outputs are empty in a shot without a key: the subject of one scene is not in the next.")

    def propagate(self, image, mask, key_frames="0", levels=4, search=2, smooth=8, anchor=_both.DEFAULT_ANCHOR,
                  occlusion=_both.DEFAULT_OCCLUSION, shots=None):
        keys = self._checked(image, key_frames, anchor, occlusion)
        ranges = self._ranges(shots, int(image.shape[0]))
        dev = node_device(image)
        out, hidden = _shots.propagate_keys_anchored_visible_shots(image.to(dev), mask.to(dev), ranges, keys, int(levels), int(search),
                                                                   int(smooth), int(anchor), int(occlusion))
        return (out.to(mask.device), hidden.to(mask.device))


NODE_CLASS_MAPPINGS = {
    "LanPaint_VideoMaskPropagateKeysAnchoredVisible": LanPaint_VideoMaskPropagateKeysAnchoredVisible,
    "LanPaint_VideoMaskPropagateKeysAnchoredVisibleShots": LanPaint_VideoMaskPropagateKeysAnchoredVisibleShots,
}
NODE_DISPLAY_NAME_MAPPINGS = {
    "LanPaint_VideoMaskPropagateKeysAnchoredVisible": "LanPaint Video Mask Propagate (Keys, Anchored, Visible)",
    "LanPaint_VideoMaskPropagateKeysAnchoredVisibleShots": "LanPaint Video Mask Propagate (Keys, Anchored, Visible, Shots)",
}
