"""LanPaint_VideoTemporalSmooth: what the sampler put under the mask of a video stops boiling from frame to frame.

The sampler invents the content under the mask frame by frame, and the colour match, the stitches, the multiband blend and the
grain match behind it treat a frame on its own.  The first defect one sees in a video inpaint is therefore that the inpainted
area boils: texture that should be one piece of background changes from frame to frame.  This node (lanpaint_amd.temporal_smooth,
on the HIP device) follows the picture's motion from every masked pixel a few frames into the past and the future, looks at what
the sampler put at the same scene point there, and pulls the pixel towards the weighted mean of what agrees with it.  It stands
behind the decode or the stitch and in front of the blend and the grain:

    ImageDecode / DetailerStitch* -> VideoTemporalSmooth -> MultibandBlend -> GrainMatch

Grain is synthesized afterwards, which is why smoothing it away here is wanted.  A single outlier frame keeps its value, because
every neighbour is rejected; the mask edge is hard (the multiband blend follows).  Host tensors in and out like the other nodes.
The reference has no such node.  LanPaint_VideoTemporalSmoothRobust (lanpaint_amd.temporal_smooth_robust_nodes) is the robust form:
it repairs the outlier frame.

This module has its own NODE_CLASS_MAPPINGS: merge them with the others' (INTEGRATION.md section 2(b)).
"""
from __future__ import annotations

import torch

from . import temporal_smooth as _temporal_smooth
from ._hostcall import node_device
from .temporal_fill_nodes import LanPaint_VideoTemporalFill


class LanPaint_VideoTemporalSmooth:
    """Pull the masked area of every video frame towards what its neighbouring frames hold at the same scene point."""

    @classmethod
    def INPUT_TYPES(s):
        field = LanPaint_VideoTemporalFill.INPUT_TYPES()["required"]
        return {"required": {
            "image": ("IMAGE", {"tooltip": "The inpainted video, one frame per batch entry."}),
            "mask": ("MASK", {"tooltip": "What was inpainted: one mask per video frame, or one mask for every frame. "
                                         "Binarised at 0.5. Nothing outside it changes."}),
            "radius": ("INT", {"default": 2, "min": 1, "max": _temporal_smooth.MAX_RADIUS, "step": 1,
                               "tooltip": "Frames looked at on either side, weighted binomially. More removes more flicker and "
                                          "follows the motion further, where it is less sure."}),
            "tolerance": ("INT", {"default": 24, "min": 0, "max": 255, "step": 1,
                                  "tooltip": "The most grey levels (of 255) a neighbouring frame's value may lie away from the "
                                             "pixel in any channel and still count. Protects against ghosts; 0 changes nothing."}),
            "motion": (list(_temporal_smooth.MOTIONS), {"default": "background",
                                                         "tooltip": "background: the motion is measured outside the mask and "
                                                                    "continued across it, for an inpainted background. picture: "
                                                                    "every pixel weighs in, for an inpainted subject that moves "
                                                                    "on its own."}),
            "levels": field["levels"],
            "search": field["search"],
            "smooth": field["smooth"],
        }}

    RETURN_TYPES = ("IMAGE", "MASK")
    RETURN_NAMES = ("image", "support")
    FUNCTION = "smooth"
    CATEGORY = "image"
    DESCRIPTION = ("Removes the frame-to-frame boiling of an inpainted video area: every masked pixel follows the picture's motion "
                   "a few frames into the past and the future and is pulled towards the weighted mean of what the neighbouring "
                   "frames hold at the same scene point, as far as that agrees with it within `tolerance`. Put it behind the decode "
                   "or the Detailer stitch and in front of the multiband blend and the grain match: grain is synthesized "
                   "afterwards. `support` is the share of the neighbouring frames that counted, 0 outside the mask. A single "
                   "outlier frame keeps its value; LanPaint_VideoTemporalSmoothRobust repairs it.")

    def smooth(self, image, mask, radius=2, tolerance=24, motion="background", levels=4, search=2, smooth=8):
        dev = node_device(image)
        out, support = _temporal_smooth.temporal_smooth(image.to(dev), mask.to(dev), int(radius), int(tolerance), motion, int(levels),
                                                        int(search), int(smooth))
        share = torch.clamp(support, min=0).to(torch.float32) / float(2 * int(radius))
        return (out.to(image.device), share.to(mask.device))


NODE_CLASS_MAPPINGS = {"LanPaint_VideoTemporalSmooth": LanPaint_VideoTemporalSmooth}
NODE_DISPLAY_NAME_MAPPINGS = {"LanPaint_VideoTemporalSmooth": "LanPaint Video Temporal Smooth"}
