"""LanPaint_DetailerCrop / LanPaint_DetailerStitch: inpaint at the resolution of the masked region.

The crop node finds the mask's bounding box, grows it by `context` and `padding`, snaps it to the latent grid, and hands the
sampler the region of image and mask at a chosen working size; the stitch node resamples the inpainted region back and
blends it into the original with a MaskBlend-style boundary, leaving every pixel outside the region untouched.  They sit
either side of LanPaint_ImageEncode / LanPaint_ImageDecode:

    image, mask -> DetailerCrop -> ImageEncode -> sampler -> ImageDecode (no image input) -> DetailerStitch -> image

Host tensors in and out like the other nodes; the per-pixel work runs on the HIP device (lanpaint_amd.detail).  The reference
has no such node (its README lists it as an open item).

This module has its own NODE_CLASS_MAPPINGS: merge them with lanpaint_amd.nodes' (INTEGRATION.md section 2(b)).
"""
from __future__ import annotations

from . import detail
from ._hostcall import node_device, node_mask


def _on_device(image, mask):
    """What every crop node starts with: (image, mask as [B, H, W]) on the HIP device the crop runs on."""
    dev = node_device(image)
    return image.to(dev), node_mask(mask, dev)


class LanPaint_DetailerCrop:
    """Crop image and mask to the masked region (one region for every frame of the batch) at a working size."""

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {
            "image": ("IMAGE", {"tooltip": "The image (or the frames of a video) to inpaint."}),
            "mask": ("MASK", {"tooltip": "The inpainting mask (1 = regenerate). Its bounding box over all frames is the region."}),
            "context": ("FLOAT", {"default": 1.5, "min": 1.0, "max": 8.0, "step": 0.001,
                                  "tooltip": "Grow the region to this multiple of the mask's bounding box, so the model sees surroundings."}),
            "padding": ("INT", {"default": 32, "min": 0, "max": 4096, "step": 1,
                                "tooltip": "Extra pixels added on every side of the region."}),
            "target": ("INT", {"default": 1024, "min": 0, "max": 8192, "step": 8,
                               "tooltip": "Long side of the working resolution; 0 keeps the region's own size (no resample)."}),
            "multiple_of": ("INT", {"default": 8, "min": 1, "max": 128, "step": 1,
                                    "tooltip": "Region and working size are multiples of this (the VAE's downscale factor)."}),
            "filter": (list(detail.FILTERS), {"default": "bicubic", "tooltip": "Antialiased resampling filter, both ways."}),
        }}

    RETURN_TYPES = ("IMAGE", "MASK", "LANPAINT_STITCH")
    RETURN_NAMES = ("cropped_image", "cropped_mask", "stitch")
    FUNCTION = "crop"
    CATEGORY = "image"
    DESCRIPTION = ("Crop image and mask to the masked region, grown by context and padding, at a chosen working resolution. "
                   "Feed the outputs to LanPaint_ImageEncode and the stitch output to LanPaint_DetailerStitch.")

    def crop(self, image, mask, context=1.5, padding=32, target=1024, multiple_of=8, filter="bicubic"):
        img, m = _on_device(image, mask)
        region = detail.plan_region(detail.mask_bbox(m), img.shape[1], img.shape[2], context, padding, multiple_of, target)
        cimg, cmask = detail.crop_resample(img, m, region, filter)
        stitch = {"original": image, "mask": mask, "region": region, "filter": filter}
        return (cimg.to(image.device), cmask.to(mask.device), stitch)


class LanPaint_DetailerStitch:
    """Resample the inpainted region back and blend it into the original; outside the region the original is untouched.  The other
    three stitch nodes subclass it and name their socket, crop node, texts, the stitch dict's key for the windows and the call."""
    STITCH_TYPE, CROP_NODE, WINDOWS, CALL = "LANPAINT_STITCH", "LanPaint_DetailerCrop", "region", staticmethod(detail.stitch)
    IMAGE_TIP = "The inpainted region, at the working resolution."
    DESCRIPTION = "Stitch the inpainted region from LanPaint_DetailerCrop back into the original image."
    RETURN_TYPES, RETURN_NAMES, FUNCTION, CATEGORY = ("IMAGE",), ("image",), "stitch", "image"

    @classmethod
    def INPUT_TYPES(s):
        blend = {"default": 9, "min": 1, "max": 51, "step": 2,
                 "tooltip": "Boundary blend width in pixels between the inpainted and original image (MaskBlend-style)."}
        return {"required": {"stitch": (s.STITCH_TYPE, {"tooltip": f"From {s.CROP_NODE}."}),
                             "image": ("IMAGE", {"tooltip": s.IMAGE_TIP}), "blend_overlap": ("INT", blend)}}

    def stitch(self, stitch, image, blend_overlap=9):
        original = stitch["original"]
        dev = node_device(original)
        labels = (stitch["labels"].to(dev),) if "labels" in stitch else ()        # after the windows, where the crop node left some
        out = self.CALL(original.to(dev), image.to(dev), stitch["mask"].to(dev), stitch[self.WINDOWS], *labels, blend_overlap,
                        stitch["filter"])
        return (out.to(original.device),)


NODE_CLASS_MAPPINGS = {"LanPaint_DetailerCrop": LanPaint_DetailerCrop, "LanPaint_DetailerStitch": LanPaint_DetailerStitch}
NODE_DISPLAY_NAME_MAPPINGS = {"LanPaint_DetailerCrop": "LanPaint Detailer Crop", "LanPaint_DetailerStitch": "LanPaint Detailer Stitch"}
