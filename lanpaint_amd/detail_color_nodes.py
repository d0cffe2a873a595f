"""LanPaint_DetailerColorMatch: bring a detailed crop's tone back to the original crop's before it is stitched.

A crop comes back from resample, VAE, sampler and VAE with a small gain and offset per channel; the stitch hides the seam but
not the drift inside the mask, and on video the drift changes from frame to frame.  This node measures both crops outside the
mask, `margin` pixels away from it, fits one gain and offset per image and channel -- pooled over `smooth` frames of a clip --
and applies it (lanpaint_amd.detail_color).  It sits between decode and any of the three stitch nodes and takes the crop node's
own outputs:

    image, mask -> DetailerCrop* -> ImageEncode -> sampler -> ImageDecode -> DetailerColorMatch -> DetailerStitch*
                        |  cropped_image, cropped_mask                              ^
                        +-----------------------------------------------------------+

For LanPaint_DetailerCropRegions, whose batch is region-major, set `clip_frames` to the number of frames per region so that
pooling never crosses regions.  Host tensors in and out like the other nodes; the per-pixel work runs on the HIP device.  The
reference has no such node.

This module has its own NODE_CLASS_MAPPINGS: merge them with the others' (INTEGRATION.md section 2(b)).
"""
from __future__ import annotations

from . import detail_color
from ._hostcall import node_device


class LanPaint_DetailerColorMatch:
    """Match the decoded windows' per-channel mean (and spread) to the original crop's, measured outside the mask."""

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {
            "image": ("IMAGE", {"tooltip": "The decoded windows, at the working resolution."}),
            "reference": ("IMAGE", {"tooltip": "cropped_image of the Detailer crop node the windows came from."}),
            "mask": ("MASK", {"tooltip": "cropped_mask of the same crop node. Statistics are taken where it is at most 0.5."}),
            "method": (list(detail_color.METHODS), {"default": "mean_std",
                                                    "tooltip": "mean_std fits gain and offset per channel, mean the offset only."}),
            "strength": ("FLOAT", {"default": 1.0, "min": 0.0, "max": 1.0, "step": 0.05,
                                   "tooltip": "Blend between the decoded windows (0) and the fully matched ones (1)."}),
            "margin": ("INT", {"default": 8, "min": 0, "max": detail_color.MAX_MARGIN, "step": 1,
                               "tooltip": "Keep the statistics this many pixels away from the mask, where the decode bleeds."}),
            "smooth": ("INT", {"default": 1, "min": 0, "max": 129, "step": 1,
                               "tooltip": "Number of frames one fit is pooled over (odd); 0 = one fit for the whole clip."}),
            "clip_frames": ("INT", {"default": 0, "min": 0, "max": 65535, "step": 1,
                                    "tooltip": "Frames per clip; 0 = the batch is one clip. For the per-region crop: the number "
                                               "of frames per region, so that pooling never crosses regions."}),
        }}

    RETURN_TYPES = ("IMAGE",)
    RETURN_NAMES = ("image",)
    FUNCTION = "match"
    CATEGORY = "image"
    DESCRIPTION = ("Match the tone of the decoded Detailer windows to the original crops, measured outside the mask. Place it "
                   "between LanPaint_ImageDecode and any LanPaint_DetailerStitch node.")

    def match(self, image, reference, mask, method="mean_std", strength=1.0, margin=8, smooth=1, clip_frames=0):
        dev = node_device(image)
        out = detail_color.match(image.to(dev), reference.to(dev), mask.to(dev), method, strength, margin, smooth, clip_frames)
        return (out.to(image.device),)


NODE_CLASS_MAPPINGS = {"LanPaint_DetailerColorMatch": LanPaint_DetailerColorMatch}
NODE_DISPLAY_NAME_MAPPINGS = {"LanPaint_DetailerColorMatch": "LanPaint Detailer Color Match"}
