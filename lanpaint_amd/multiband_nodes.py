"""LanPaint_MultibandBlend: a Laplacian-pyramid seam between an original image and a generated one.

Every stitch and decode ends in MaskBlend's rule, one feather of at most 51 pixels (`blend_overlap`).  What low-frequency
difference is left between the two images -- shading, a gradient, a vignette -- shows as a step in a narrow band, and a wide
band ghosts fine texture.  This node blends every frequency band over a width in proportion to its wavelength
(lanpaint_amd.multiband: the Burt-Adelson blend on the HIP device).  It goes after any stitch or decode:

    DetailerStitch(blend_overlap = 1) -> image2 ---+
    the original image -> image1 ------------------+-> MultibandBlend -> image
    the mask --------------------------------------+

    ImageDecode(blend_overlap = 1) -> image2, the original -> image1, the mask -> MultibandBlend -> image

`levels` is the reach: no pixel further than 2^(levels + 2) - 4 from the mask changes, 124 pixels at the default of 5.
Host tensors in and out like the other nodes.  The reference has no such node.

This module has its own NODE_CLASS_MAPPINGS: merge them with the others' (INTEGRATION.md section 2(b)).
"""
from __future__ import annotations

from . import multiband as _multiband
from ._hostcall import node_device, node_mask


class LanPaint_MultibandBlend:
    """Blend image2 into image1 through the mask, each frequency band over its own width."""

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {
            "image1": ("IMAGE", {"tooltip": "The image that is kept where the mask is 0 (the original)."}),
            "image2": ("IMAGE", {"tooltip": "The image that is shown where the mask is 1 (the stitched or decoded one)."}),
            "mask": ("MASK", {"tooltip": "Soft values are used as given; nothing is binarised or dilated."}),
            "levels": ("INT", {"default": 5, "min": 0, "max": 12, "step": 1,
                               "tooltip": "Pyramid levels: nothing further than 2^(levels + 2) - 4 pixels from the mask changes; "
                                          "0 is a plain blend through the mask."}),
        }}

    RETURN_TYPES = ("IMAGE",)
    RETURN_NAMES = ("image",)
    FUNCTION = "blend"
    CATEGORY = "image"
    DESCRIPTION = ("Laplacian-pyramid blend of two images through a mask. Stitch or decode with blend_overlap 1, then blend the "
                   "original (image1) and the result (image2) here.")

    def blend(self, image1, image2, mask, levels=5):
        dev = node_device(image1)
        out = _multiband.blend_multiband(image1.to(dev), image2.to(dev), node_mask(mask, dev), int(levels))
        return (out.to(image1.device),)


NODE_CLASS_MAPPINGS = {"LanPaint_MultibandBlend": LanPaint_MultibandBlend}
NODE_DISPLAY_NAME_MAPPINGS = {"LanPaint_MultibandBlend": "LanPaint Multiband Blend"}
