"""LanPaint_VideoMaskPropagateKeys: masks painted on several frames of a clip follow the picture's motion and are merged between
the keys.

LanPaint_VideoMaskPropagate carries one painted mask through the clip and drifts with the distance from it; the video mask editor
morphs between painted keyframes without looking at the picture.  This node does both (lanpaint_amd.propagate_keys, on the HIP
device): every key is carried along the motion in both directions, and between two keys the two carried masks are merged through
their signed distance fields with weights that move from one key to the other.  The result equals the painted mask on every key
frame, so a user who sees drift paints one more key instead of restarting.  It takes the same place in the chain:

    painted masks + the video -> VideoMaskPropagateKeys -> VideoMaskStabilize -> MaskRefine -> ImageEncode / DetailerCrop*

Occlusion is not handled.  Host tensors in and out like the other nodes.  The reference has no such node.

This module has its own NODE_CLASS_MAPPINGS: merge them with the others' (INTEGRATION.md section 2(b)).
"""
from __future__ import annotations

import re

from . import propagate_keys as _keys
from ._hostcall import node_device
from .propagate_nodes import MATCHER_WIDGETS


def parse_key_frames(text):
    """"0, 12 40" -> [0, 12, 40]: integers separated by commas and/or blanks."""
    if not isinstance(text, str):
        raise ValueError(f"key_frames must be a string of integers, got {text!r}")
    words = [w for w in re.split(r"[,\s]+", text.strip()) if w]
    for w in words:
        if not re.fullmatch(r"[+-]?\d+", w):
            raise ValueError(f"key_frames holds {w!r}: integers separated by commas or blanks")
    return [int(w) for w in words]


class LanPaint_VideoMaskPropagateKeys:
    """Carry masks painted on several frames through the video along the picture's motion and merge them between the keys."""

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {
            "image": ("IMAGE", {"tooltip": "The video, one frame per batch entry."}),
            "mask": ("MASK", {"tooltip": "The painted masks: one per key frame in the order of key_frames, or one per video frame "
                                         "of which only the key frames' are read. Binarised at 0.5."}),
            "key_frames": ("STRING", {"default": "0",
                                      "tooltip": "The frames the masks were painted on: increasing integers separated by commas "
                                                 "or blanks, each a frame of the video."}),
            **MATCHER_WIDGETS,
        }}

    RETURN_TYPES = ("MASK",)
    RETURN_NAMES = ("mask",)
    FUNCTION = "propagate"
    CATEGORY = "mask"
    DESCRIPTION = ("Makes a per-frame video mask from masks painted on several key frames: every key follows the picture's "
                   "motion in both directions, and between two keys the two carried masks are merged through their distance "
                   "fields, so the result equals the painting on every key and drift is pulled back there. Paint one more key "
                   "where the mask drifts. Put it in front of the video mask stabilize, the mask refine, the encode and the "
                   "Detailer crops. Occlusion is not handled; an empty key means nothing is there.")

    def propagate(self, image, mask, key_frames="0", levels=4, search=2, smooth=8):
        keys = parse_key_frames(key_frames)
        _keys.chain_plan(int(image.shape[0]), keys)                  # bad keys are refused before a device is looked for
        dev = node_device(image)
        out = _keys.propagate_keys(image.to(dev), mask.to(dev), keys, int(levels), int(search), int(smooth))
        return (out.to(mask.device),)


NODE_CLASS_MAPPINGS = {"LanPaint_VideoMaskPropagateKeys": LanPaint_VideoMaskPropagateKeys}
NODE_DISPLAY_NAME_MAPPINGS = {"LanPaint_VideoMaskPropagateKeys": "LanPaint Video Mask Propagate (Keys)"}
