"""LanPaint_VideoMaskStabilize: take the flicker out of a per-frame video mask.

A mask that a segmenter made frame by frame, or that was painted frame by frame, flickers: its edge jitters by a pixel or two and
single frames come back empty or with a stray blob.  This node filters the mask's signed distance field along time
(lanpaint_amd.stabilize, on the HIP device): a temporal median drops what lasts at most `median_radius` frames, a binomial
smoothing of radius `smooth_radius` calms the edge.  It goes behind whatever makes the per-frame mask and in front of whatever
reads it:

    a per-frame segmenter / VideoMaskEditor -> mask -> VideoMaskStabilize -> MaskRefine -> ImageEncode / DetailerCrop*

Host tensors in and out like the other nodes.  The reference has no such node.

This module has its own NODE_CLASS_MAPPINGS: merge them with the others' (INTEGRATION.md section 2(b)).
"""
from __future__ import annotations

from . import stabilize as _stabilize
from ._hostcall import node_device


class LanPaint_VideoMaskStabilize:
    """Median and smooth a video mask's signed distance field along time."""

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {
            "mask": ("MASK", {"tooltip": "The per-frame mask of a video, one frame per batch entry: from a per-frame segmenter, "
                                         "painted frame by frame, or from the video mask editor. Binarised at 0.5."}),
            "median_radius": ("INT", {"default": 1, "min": 0, "max": 3, "step": 1,
                                      "tooltip": "Frames on either side that vote on every pixel: an empty frame, a dropout or a "
                                                 "stray blob that lasts at most this many frames disappears. 0 switches the median "
                                                 "off."}),
            "smooth_radius": ("INT", {"default": 2, "min": 0, "max": 8, "step": 1,
                                      "tooltip": "Frames on either side whose edge position is averaged (binomial weights): calms an "
                                                 "edge that jitters. Smoothing without the median does not repair dropped frames; "
                                                 "keep median_radius at 1 or more for that."}),
            "grow": ("FLOAT", {"default": 0.0, "min": -256.0, "max": 256.0, "step": 0.25,
                               "tooltip": "Pixels to move the stabilized edge outwards (positive) or inwards (negative)."}),
            "feather": ("FLOAT", {"default": 0.0, "min": 0.0, "max": 64.0, "step": 0.25,
                                  "tooltip": "Half-width in pixels of a linear ramp across the edge; 0 gives a hard 0 / 1 mask."}),
        }}

    RETURN_TYPES = ("MASK",)
    RETURN_NAMES = ("mask",)
    FUNCTION = "stabilize"
    CATEGORY = "mask"
    DESCRIPTION = ("Takes the flicker out of a per-frame video mask: a temporal median and a binomial smoothing of its signed "
                   "distance field. Put it behind a per-frame segmenter or the video mask editor and in front of the mask refine, "
                   "the encode and the Detailer crops. Smoothing alone does not repair dropped frames; the median does.")

    def stabilize(self, mask, median_radius=1, smooth_radius=2, grow=0.0, feather=0.0):
        dev = node_device(mask)
        out = _stabilize.stabilize_masks(mask.to(dev), int(median_radius), int(smooth_radius), float(grow), float(feather))
        return (out.to(mask.device),)


NODE_CLASS_MAPPINGS = {"LanPaint_VideoMaskStabilize": LanPaint_VideoMaskStabilize}
NODE_DISPLAY_NAME_MAPPINGS = {"LanPaint_VideoMaskStabilize": "LanPaint Video Mask Stabilize"}
