"""LanPaint_VideoTemporalFill: what lies under the mask of a video frame is borrowed from the nearest frame that shows it.

The mask nodes make a per-frame mask and the Detailer, blend and grain nodes finish an inpaint; under the mask the only fill was
LanPaint_MaskFill, which continues every frame's surroundings into its hole and knows nothing of the other frames.  When a
subject moves across a background, or the camera pans past it, most of what the mask covers in one frame is plain background a
few frames earlier or later.  This node takes it from there (lanpaint_amd.temporal_fill, on the HIP device): the motion of the
unmasked picture is measured by a block matching and continued across the hole, and every masked pixel is sampled once from the
nearest frame in which it is visible.  It stands between the mask chain and the spatial fill:

    mask chain -> VideoTemporalFill -> (remaining mask) MaskFill -> ImageEncode / DetailerCrop*

Borrowed pixels are not colour-matched (DetailerColorMatch exists) and not checked against their surroundings.  Host tensors in
and out like the other nodes.  The reference has no such node.

This module has its own NODE_CLASS_MAPPINGS: merge them with the others' (INTEGRATION.md section 2(b)).
"""
from __future__ import annotations

import torch

from . import temporal_fill as _temporal_fill
from ._hostcall import node_device


class LanPaint_VideoTemporalFill:
    """Fill the masked area of every video frame with the background another frame shows there."""

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {
            "image": ("IMAGE", {"tooltip": "The video, one frame per batch entry."}),
            "mask": ("MASK", {"tooltip": "What to remove: one mask per video frame, or one mask for every frame. "
                                         "Binarised at 0.5."}),
            "levels": ("INT", {"default": 4, "min": 1, "max": 6, "step": 1,
                               "tooltip": "Pyramid levels of the motion search. Every level doubles the background motion per "
                                          "frame that can be followed: about search * 2^levels pixels."}),
            "search": ("INT", {"default": 2, "min": 1, "max": 7, "step": 1,
                               "tooltip": "Pixels searched around the coarser level's motion at every level. More follows "
                                          "faster or less regular motion and costs time with its square."}),
            "smooth": ("INT", {"default": 8, "min": 0, "max": 64, "step": 1,
                               "tooltip": "The price of a pixel of displacement in the match, in grey levels summed over a block: "
                                          "keeps flat, textureless areas from drifting. 0 switches it off."}),
            "reach": ("INT", {"default": 0, "min": 0, "max": 65535, "step": 1,
                              "tooltip": "The most frames away a pixel may be borrowed from. Near frames match the light and the "
                                         "grain better; far frames fill more. 0 allows the whole clip."}),
        }}

    RETURN_TYPES = ("IMAGE", "MASK", "MASK")
    RETURN_NAMES = ("image", "remaining", "filled")
    FUNCTION = "fill"
    CATEGORY = "image"
    DESCRIPTION = ("Fills the masked area of a video from its other frames: the background's motion is measured by a block "
                   "matching outside the mask, and every masked pixel is taken from the nearest frame that shows it. The result "
                   "is temporally consistent and leaves the sampler less to invent. Put it behind the video mask nodes and in "
                   "front of the mask fill, the encode and the Detailer crops; give `remaining` to them as the mask. What no "
                   "frame shows, such as a subject that never moves, stays in `remaining`. Borrowed pixels are not colour-matched.")

    def fill(self, image, mask, levels=4, search=2, smooth=8, reach=0):
        dev = node_device(image)
        filled, remaining, source = _temporal_fill.temporal_fill(image.to(dev), mask.to(dev), int(levels), int(search), int(smooth),
                                                                 int(reach))
        frames = torch.arange(source.shape[0], dtype=torch.int32, device=dev).view(-1, 1, 1)
        borrowed = ((source >= 0) & (source != frames)).to(torch.float32)          # the mask's bits without `remaining`
        return (filled.to(image.device), remaining.to(mask.device), borrowed.to(mask.device))


NODE_CLASS_MAPPINGS = {"LanPaint_VideoTemporalFill": LanPaint_VideoTemporalFill}
NODE_DISPLAY_NAME_MAPPINGS = {"LanPaint_VideoTemporalFill": "LanPaint Video Temporal Fill"}
