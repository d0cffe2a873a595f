"""LanPaint_VideoMaskPropagate: one mask painted on one frame of a clip follows the picture's motion through the other frames.

The video mask editor morphs between painted keyframes and follows a subject's centroid, not its outline; the stabilize and the
mask refine take the per-frame mask as given.  This node makes that per-frame mask from one painted frame
(lanpaint_amd.propagate, on the HIP device): a block matching weighted by the mask measures the motion from frame to frame, and
the key mask is sampled through the accumulated motion.  It is the first link of the video mask chain:

    one painted mask + the video -> VideoMaskPropagate -> VideoMaskStabilize -> MaskRefine -> ImageEncode / DetailerCrop*

One keyframe only; nothing handles occlusion or re-anchors against drift (propagate_anchored_nodes.py does the latter).  Host
tensors in and out like the other nodes.  The reference has no such node.

This module has its own NODE_CLASS_MAPPINGS: merge them with the others' (INTEGRATION.md section 2(b)).
"""
from __future__ import annotations

from . import propagate as _propagate
from ._hostcall import node_device

# The block matcher's three widgets, as every propagate node shows them: spliced into INPUT_TYPES where they stood.
MATCHER_WIDGETS = {
    "levels": ("INT", {"default": 4, "min": 1, "max": 6, "step": 1,
                       "tooltip": "Pyramid levels of the motion search. Every level doubles the motion per frame that can "
                                  "be followed: about search * 2^levels pixels."}),
    "search": ("INT", {"default": 2, "min": 1, "max": 7, "step": 1,
                       "tooltip": "Pixels searched around the coarser level's motion at every level. More follows "
                                  "faster or less regular motion and costs time with its square."}),
    "smooth": ("INT", {"default": 8, "min": 0, "max": 64, "step": 1,
                       "tooltip": "The price of a pixel of displacement in the match, in grey levels summed over a block: "
                                  "keeps flat, textureless areas from drifting. 0 switches it off."}),
}

class LanPaint_VideoMaskPropagate:
    """Carry a mask painted on one frame through the video along the picture's motion."""

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {
            "image": ("IMAGE", {"tooltip": "The video, one frame per batch entry."}),
            "mask": ("MASK", {"tooltip": "The mask painted on the key frame: one frame, or one per video frame of which only the "
                                         "key frame's is read. Binarised at 0.5."}),
            "key_frame": ("INT", {"default": 0, "min": 0, "max": 65534, "step": 1,
                                  "tooltip": "The frame the mask was painted on. The mask is carried forwards and backwards "
                                             "from it; it must be a frame of the video."}),
            **MATCHER_WIDGETS,
        }}

    RETURN_TYPES = ("MASK",)
    RETURN_NAMES = ("mask",)
    FUNCTION = "propagate"
    CATEGORY = "mask"
    DESCRIPTION = ("Makes a per-frame video mask from one mask painted on one frame: the mask follows the picture's motion, "
                   "measured by a block matching under the mask. Put it in front of the video mask stabilize, the mask refine, "
                   "the encode and the Detailer crops. One keyframe; occlusion is not handled and a long clip may drift.")

    def propagate(self, image, mask, key_frame=0, levels=4, search=2, smooth=8):
        dev = node_device(image)
        out = _propagate.propagate_masks(image.to(dev), mask.to(dev), int(key_frame), int(levels), int(search), int(smooth))
        return (out.to(mask.device),)


NODE_CLASS_MAPPINGS = {"LanPaint_VideoMaskPropagate": LanPaint_VideoMaskPropagate}
NODE_DISPLAY_NAME_MAPPINGS = {"LanPaint_VideoMaskPropagate": "LanPaint Video Mask Propagate"}
