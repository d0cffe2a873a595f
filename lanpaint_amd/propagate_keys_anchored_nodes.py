"""LanPaint_VideoMaskPropagateKeysAnchored: masks painted on several frames follow the picture's motion, each matched against its
own key frame again on every frame, and are merged between the keys.

LanPaint_VideoMaskPropagateKeys pins the mask to every painting, but half way through a long gap both carried masks have fallen
behind a subject that moves a fraction of a pixel per frame.  This node (lanpaint_amd.propagate_keys_anchored, on the HIP device)
gives every chain LanPaint_VideoMaskPropagateAnchored's correction: each frame is compared with the key frame's picture carried
along the same motion, and the carried mask is moved by what the comparison finds.  It sits where the keys node sits:

    painted masks + the video -> VideoMaskPropagateKeysAnchored -> VideoMaskStabilize -> MaskRefine -> ImageEncode / DetailerCrop*

Occlusion is not handled.  Host tensors in and out like the other nodes.  The reference has no such node.

This module has its own NODE_CLASS_MAPPINGS: merge them with the others' (INTEGRATION.md section 2(b)).
"""
from __future__ import annotations

from . import propagate_keys as _keys
from . import propagate_keys_anchored as _anchored
from ._hostcall import int_in, node_device
from .propagate_keys_nodes import parse_key_frames
from .propagate_nodes import MATCHER_WIDGETS


class LanPaint_VideoMaskPropagateKeysAnchored:
    """Carry masks painted on several frames through the video, each re-matched against its key frame, merged between the keys."""

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
            "anchor": ("INT", {"default": _anchored.DEFAULT_ANCHOR, "min": 0, "max": _anchored.MAX_ANCHOR, "step": 1,
                               "tooltip": "Pixels searched around the carried position when a frame is matched against its key "
                                          "frame: the largest error one frame can take out. It costs time with its square; 0 "
                                          "switches the correction off."}),
        }}

    RETURN_TYPES = ("MASK",)
    RETURN_NAMES = ("mask",)
    FUNCTION = "propagate"
    CATEGORY = "mask"
    DESCRIPTION = ("Makes a per-frame video mask from masks painted on several key frames, like the video mask propagate from "
                   "keys: every key follows the picture's motion in both directions and the two carried masks are merged between "
                   "two keys. Every frame is also matched against its key frame again, so the mask does not fall behind its "
                   "subject half way through a long gap. Put it in front of the video mask stabilize, the mask refine, the encode "
                   "and the Detailer crops. Occlusion is not handled; an empty key means nothing is there; a subject that stops "
                   "looking like its key frame drifts as before.")

    def propagate(self, image, mask, key_frames="0", levels=4, search=2, smooth=8, anchor=_anchored.DEFAULT_ANCHOR):
        keys = parse_key_frames(key_frames)
        _keys.chain_plan(int(image.shape[0]), keys)                  # bad keys are refused before a device is looked for
        int_in(int(anchor), 0, _anchored.MAX_ANCHOR, "anchor")
        dev = node_device(image)
        out = _anchored.propagate_keys_anchored(image.to(dev), mask.to(dev), keys, int(levels), int(search), int(smooth), int(anchor))
        return (out.to(mask.device),)


NODE_CLASS_MAPPINGS = {"LanPaint_VideoMaskPropagateKeysAnchored": LanPaint_VideoMaskPropagateKeysAnchored}
NODE_DISPLAY_NAME_MAPPINGS = {"LanPaint_VideoMaskPropagateKeysAnchored": "LanPaint Video Mask Propagate (Keys, Anchored)"}
