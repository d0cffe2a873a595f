"""LanPaint_OutpaintPad and LanPaint_MaskFill: decide what lies under the mask before LanPaint_ImageEncode.

The VAE encoder's receptive field reaches across the mask's edge, so a flat border on an extended canvas, or an unwanted object
under an inpaint mask, leaks into the known latent next to the edge.  Both nodes put a smooth continuation of the known pixels
there instead (lanpaint_amd.fill: a push-pull pyramid on the HIP device):

    image -> OutpaintPad -> ImageEncode -> sampler -> ImageDecode(image = padded image, mask) -> image
                  |  image, mask                            ^
                  +-----------------------------------------+

    image, mask -> MaskFill -> ImageEncode -> sampler -> ImageDecode(image = the original image, mask) -> image

LanPaint_ImageDecode still merges against the original (or padded) image, so the fill only ever shows through the encoder.
Host tensors in and out like the other nodes.  The reference has no such nodes.

This module has its own NODE_CLASS_MAPPINGS: merge them with the others' (INTEGRATION.md section 2(b)).
"""
from __future__ import annotations

from . import fill as _fill
from ._hostcall import node_device, node_mask


class LanPaint_OutpaintPad:
    """Extend the canvas, mask the new area and a band of the original along it, and fill what is masked from the original."""

    @classmethod
    def INPUT_TYPES(s):
        pad = {"default": 0, "min": 0, "max": 8192, "step": 8}
        return {"required": {
            "image": ("IMAGE", {"tooltip": "The image to extend."}),
            "left": ("INT", {**pad, "tooltip": "Pixels to add on the left; grown until the canvas is a multiple of multiple_of."}),
            "top": ("INT", {**pad, "tooltip": "Pixels to add at the top."}),
            "right": ("INT", {**pad, "tooltip": "Pixels to add on the right."}),
            "bottom": ("INT", {**pad, "tooltip": "Pixels to add at the bottom."}),
            "overlap": ("INT", {"default": 16, "min": 0, "max": 512, "step": 1,
                                "tooltip": "Band of the original, along every padded side, that is regenerated too."}),
            "multiple_of": ("INT", {"default": 8, "min": 1, "max": 128, "step": 1,
                                    "tooltip": "The canvas's padded sides are brought up to a multiple of this."}),
            "fill": ("BOOLEAN", {"default": True,
                                 "tooltip": "Fill the masked area from the original; off leaves zeros there."}),
        }, "optional": {
            "mask": ("MASK", {"tooltip": "A mask on the original image; it is kept (soft values too) inside the canvas's mask."}),
        }}

    RETURN_TYPES = ("IMAGE", "MASK")
    RETURN_NAMES = ("image", "mask")
    FUNCTION = "pad"
    CATEGORY = "image"
    DESCRIPTION = ("Build an outpaint canvas and its mask. Feed both to LanPaint_ImageEncode, and the padded image and the mask "
                   "to LanPaint_ImageDecode.")

    def pad(self, image, left=0, top=0, right=0, bottom=0, overlap=16, multiple_of=8, fill=True, mask=None):
        dev = node_device(image)
        m = None if mask is None else node_mask(mask, dev)
        canvas, mask_out = _fill.outpaint_pad(image.to(dev), m, left, top, right, bottom, overlap, multiple_of,
                                              bool(fill))
        return canvas.to(image.device), mask_out.to(image.device)


class LanPaint_MaskFill:
    """Replace the masked area by a smooth continuation of its surroundings."""

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {
            "image": ("IMAGE", {"tooltip": "The image whose masked area is to be filled."}),
            "mask": ("MASK", {"tooltip": "Pixels above 0.5 are replaced; the others come back unchanged."}),
        }}

    RETURN_TYPES = ("IMAGE",)
    RETURN_NAMES = ("image",)
    FUNCTION = "fill"
    CATEGORY = "image"
    DESCRIPTION = ("Fill the masked area from the known pixels before LanPaint_ImageEncode. LanPaint_ImageDecode still merges "
                   "against the original image.")

    def fill(self, image, mask):
        dev = node_device(image)
        return (_fill.fill_masked(image.to(dev), node_mask(mask, dev)).to(image.device),)


NODE_CLASS_MAPPINGS = {"LanPaint_OutpaintPad": LanPaint_OutpaintPad, "LanPaint_MaskFill": LanPaint_MaskFill}
NODE_DISPLAY_NAME_MAPPINGS = {"LanPaint_OutpaintPad": "LanPaint Outpaint Pad", "LanPaint_MaskFill": "LanPaint Mask Fill"}
