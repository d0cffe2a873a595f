"""LanPaint_VideoMaskPropagateKeysVisible: masks painted on several frames follow the picture's motion, stay off whatever passes in
front of the subject, and are merged between the keys so that a chain that lost the subject gives way to the other.

LanPaint_VideoMaskPropagateKeys honours several painted keys and puts the mask on an occluder; LanPaint_VideoMaskPropagateVisible
keeps the mask off the occluder but has one key, and a subject that is covered entirely is lost.  This node does both
(lanpaint_amd.propagate_keys_visible, on the HIP device): paint a second key behind the occluder, and between the two keys the
frames in front of the occluder come from the first key, the frames behind it from the second, and the covered part is returned as
a second output.  It takes the same place in the chain:

    painted masks + the video -> VideoMaskPropagateKeysVisible -> VideoMaskStabilize -> MaskRefine -> ImageEncode / DetailerCrop*

Occlusion edges are as coarse as the 8 x 8 blocks, which the mask refine sharpens; a subject is not followed through a full
occlusion, the next key recovers it.  Host tensors in and out like the other nodes.  The reference has no such node.

This module has its own NODE_CLASS_MAPPINGS: merge them with the others' (INTEGRATION.md section 2(b)).
"""
from __future__ import annotations

from . import propagate_keys_visible as _kv
from ._hostcall import node_device
from .propagate_keys_nodes import LanPaint_VideoMaskPropagateKeys, parse_key_frames
from .propagate_visible_nodes import LanPaint_VideoMaskPropagateVisible


class LanPaint_VideoMaskPropagateKeysVisible:
    """Carry masks painted on several frames through the video along the picture's motion, keep them off what passes in front,
    and merge them between the keys."""

    @classmethod
    def INPUT_TYPES(s):
        required = dict(LanPaint_VideoMaskPropagateKeys.INPUT_TYPES()["required"])
        required["occlusion"] = LanPaint_VideoMaskPropagateVisible.INPUT_TYPES()["required"]["occlusion"]
        return {"required": required}

    RETURN_TYPES = ("MASK", "MASK")
    RETURN_NAMES = ("mask", "hidden")
    OUTPUT_TOOLTIPS = ("The carried and merged mask without the part that something covers: what the sampler should repaint.",
                       "The part of the subject that is behind something, frame by frame. Add it back to the mask when you want "
                       "to inpaint through the occluder; leave it out to keep the occluder as it is.")
    FUNCTION = "propagate"
    CATEGORY = "mask"
    DESCRIPTION = ("Makes a per-frame video mask from masks painted on several key frames, like the video mask propagate from "
                   "keys, and keeps it off whatever passes in front of the subject: the covered part moves from `mask` to "
                   "`hidden`. When the subject is covered entirely, paint a second key behind the occluder: between the two keys "
                   "a chain that lost the subject gives way to the other, so the frames in front of the occluder follow the first "
                   "key and the frames behind it the second. The result equals the painting on every key. Put it in front of "
                   "the video mask stabilize, the mask refine, the encode and the Detailer crops. An empty key means nothing is "
                   "there.")

    def propagate(self, image, mask, key_frames="0", levels=4, search=2, smooth=8, occlusion=_kv.DEFAULT_OCCLUSION):
        keys = parse_key_frames(key_frames)
        _kv.chain_plan(int(image.shape[0]), keys)                    # bad keys are refused before a device is looked for
        dev = node_device(image)
        out, hidden = _kv.propagate_keys_visible(image.to(dev), mask.to(dev), keys, int(levels), int(search), int(smooth),
                                                 int(occlusion))
        return (out.to(mask.device), hidden.to(mask.device))


NODE_CLASS_MAPPINGS = {"LanPaint_VideoMaskPropagateKeysVisible": LanPaint_VideoMaskPropagateKeysVisible}
NODE_DISPLAY_NAME_MAPPINGS = {"LanPaint_VideoMaskPropagateKeysVisible": "LanPaint Video Mask Propagate (Keys, Visible)"}
