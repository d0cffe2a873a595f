"""LanPaint_MaskFillPatch: fill the masked area with texture from its surroundings before LanPaint_ImageEncode.

LanPaint_MaskFill (fill_nodes.py) puts a smooth continuation under the mask; on grass, brick, fabric, foliage or gravel that is a
blur, and the blur is all the VAE encoder sees across the mask's edge -- and, with denoise < 1, where the sampler starts.  This node
copies texture from the known part of the same image instead (lanpaint_amd.fill.fill_masked_patch: a PatchMatch search and vote on
the HIP device, the same bits on every run):

    image, mask -> MaskFillPatch -> ImageEncode -> sampler -> ImageDecode(image = the original image, mask) -> image

Not for smooth shading: an exemplar fill cannot extrapolate a gradient, and LanPaint_MaskFill stays the choice there.  Frames of a
video are filled independently: LanPaint's temporal fill goes in front of this node and its temporal smooth behind it.  At most 4
channels.  Host tensors in and out like the other nodes.  The reference has no such node.

This module has its own NODE_CLASS_MAPPINGS: merge them with the others' (INTEGRATION.md section 2(b)).  It stands beside
fill_nodes.py, whose two mappings are fixed.
"""
from __future__ import annotations

from . import _cabi
from . import fill as _fill
from ._hostcall import node_device, node_mask


class LanPaint_MaskFillPatch:
    """Replace the masked area by texture copied from the known part of the image."""

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {
            "image": ("IMAGE", {"tooltip": "The image whose masked area is to be filled."}),
            "mask": ("MASK", {"tooltip": "Pixels above 0.5 are replaced; the others come back unchanged."}),
            "radius": ("INT", {"default": 3, "min": 1, "max": _cabi.LP_FILL_PATCH_MAX_RADIUS, "step": 1,
                               "tooltip": "Patch radius: patches are 2 * radius + 1 pixels a side."}),
            "levels": ("INT", {"default": _fill.AUTO, "min": _fill.AUTO, "max": _cabi.LP_FILL_PATCH_MAX_LEVELS, "step": 1,
                               "tooltip": "Pyramid levels, coarse to fine; 0 chooses as many as leave four patches a side."}),
            "iters": ("INT", {"default": 4, "min": 1, "max": _cabi.LP_FILL_PATCH_MAX_ITERS, "step": 1,
                              "tooltip": "Search and vote rounds per level."}),
            "seed": ("INT", {"default": 0, "min": 0, "max": 65535, "step": 1,
                             "tooltip": "Seed of the random search; the same seed gives the same bits."}),
        }}

    RETURN_TYPES = ("IMAGE",)
    RETURN_NAMES = ("image",)
    FUNCTION = "fill"
    CATEGORY = "image"
    DESCRIPTION = ("Fill the masked area with texture from the known pixels before LanPaint_ImageEncode. Use LanPaint_MaskFill "
                   "on smooth shading. LanPaint_ImageDecode still merges against the original image.")

    def fill(self, image, mask, radius=3, levels=_fill.AUTO, iters=4, seed=0):
        dev = node_device(image)
        out = _fill.fill_masked_patch(image.to(dev), node_mask(mask, dev), int(radius), int(levels), int(iters), int(seed))
        return (out.to(image.device),)


NODE_CLASS_MAPPINGS = {"LanPaint_MaskFillPatch": LanPaint_MaskFillPatch}
NODE_DISPLAY_NAME_MAPPINGS = {"LanPaint_MaskFillPatch": "LanPaint Mask Fill (Patch)"}
