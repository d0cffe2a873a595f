"""LanPaint_MaskRefine: grow a mask by a true distance and snap its edge onto the image's.

Every node after the sampler takes the mask as given.  A painted mask is a rough blob; a `LanPaint_VideoMaskEditor` mask between
two keyframes is the morph of two blobs and follows the subject's centroid, not its outline.  This node grows or shrinks the mask
by a Euclidean distance and then runs the colour guided filter with the image as the guide (lanpaint_amd.refine, on the HIP
device): where the image has an edge within `radius` pixels of the mask's, the mask's edge moves onto it.  For a video every
frame is refined with that frame as its guide.  It goes in front of whatever reads the mask:

    VideoMaskEditor -> mask --+
    the image or the frames --+-> MaskRefine(grow, radius, eps) -> mask -> ImageEncode / DetailerCrop* / MaskFill / MultibandBlend

Host tensors in and out like the other nodes.  The reference has no such node.

This module has its own NODE_CLASS_MAPPINGS: merge them with the others' (INTEGRATION.md section 2(b)).
"""
from __future__ import annotations

from . import refine as _refine
from ._hostcall import node_device, node_mask


class LanPaint_MaskRefine:
    """Grow or shrink the mask by a Euclidean distance, then pull its edge onto the nearest edge of the image."""

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {
            "image": ("IMAGE", {"tooltip": "The image the mask belongs to: the guide whose edges the mask's edge is pulled onto. "
                                           "For a video, the frames; every frame guides its own mask."}),
            "mask": ("MASK", {"tooltip": "The rough mask: painted by hand, or from the video mask editor. One mask for all "
                                         "images or one per image."}),
            "grow": ("INT", {"default": 0, "min": -256, "max": 256, "step": 1,
                             "tooltip": "Pixels of Euclidean distance to grow (positive) or shrink (negative) the mask by before "
                                        "the edge snap; the mask is binarised at 0.5 when this is not 0."}),
            "radius": ("INT", {"default": 8, "min": 0, "max": 64, "step": 1,
                               "tooltip": "How far, in pixels, the mask's edge may move to reach an edge of the image; nothing "
                                          "further than twice this from the mask's edge changes. 0 only grows."}),
            "eps": ("FLOAT", {"default": 1e-3, "min": 1e-6, "max": 1.0, "step": 1e-4,
                              "tooltip": "How much colour variation counts as an edge, on the [0, 1] image scale, squared: larger "
                                         "values smooth the mask more and follow the image less."}),
        }}

    RETURN_TYPES = ("MASK",)
    RETURN_NAMES = ("mask",)
    FUNCTION = "refine"
    CATEGORY = "mask"
    DESCRIPTION = ("Grows or shrinks a mask by a true Euclidean distance and snaps its edge onto the image's (colour guided "
                   "filter). Put it behind the video mask editor and in front of the encode, a Detailer crop, the mask fill or "
                   "the multiband blend.")

    def refine(self, image, mask, grow=0, radius=8, eps=1e-3):
        dev = node_device(image)
        return (_refine.refine_mask(image.to(dev), node_mask(mask, dev), int(radius), float(eps), int(grow)).to(image.device),)


NODE_CLASS_MAPPINGS = {"LanPaint_MaskRefine": LanPaint_MaskRefine}
NODE_DISPLAY_NAME_MAPPINGS = {"LanPaint_MaskRefine": "LanPaint Mask Refine"}
