"""LanPaint_DetailerCropRegions / LanPaint_DetailerStitchRegions: detail every connected masked area in a window of its own.

LanPaint_DetailerCrop takes the bounding box of the whole mask, so two masked faces at opposite corners of a frame give a
region that is nearly the frame.  These nodes split the mask into its connected components on the device, group them into at
most `max_regions` regions of one size (lanpaint_amd.detail.plan_regions) and hand the sampler all crops stacked as one batch,
region-major: `region_count` x the input's batch.  Each region's mask holds its own components only.  The stitch node puts
the regions back in order and leaves every pixel outside their windows untouched.

    image, mask -> DetailerCropRegions -> ImageEncode -> sampler -> ImageDecode (no image input) -> DetailerStitchRegions

With max_regions = 1 and min_area = 1 the pair equals LanPaint_DetailerCrop / LanPaint_DetailerStitch bit for bit.  Host
tensors in and out like the other nodes; the per-pixel work runs on the HIP device.  The reference has no such node.

This module has its own NODE_CLASS_MAPPINGS: merge them with the others' (INTEGRATION.md section 2(b)).
"""
from __future__ import annotations

from . import _cabi, detail
from .detail_nodes import LanPaint_DetailerCrop, LanPaint_DetailerStitch, _on_device


class LanPaint_DetailerCropRegions:
    """Crop image and mask to one window per connected masked area, all windows at one working size, stacked as a batch."""

    @classmethod
    def INPUT_TYPES(s):
        required = dict(LanPaint_DetailerCrop.INPUT_TYPES()["required"])
        required["mask"] = ("MASK", {"tooltip": "The inpainting mask (1 = regenerate). Its connected areas, over all frames, "
                                                "become the regions."})
        required["min_area"] = ("INT", {"default": 64, "min": 1, "max": 1 << 30, "step": 1,
                                        "tooltip": "Connected areas of fewer masked pixels are left out (and stay unchanged)."})
        required["max_regions"] = ("INT", {"default": 8, "min": 1, "max": _cabi.LP_DETAIL_MAX_REGIONS, "step": 1,
                                           "tooltip": "At most this many regions; the closest areas are merged beyond it."})
        return {"required": required}

    RETURN_TYPES = ("IMAGE", "MASK", "LANPAINT_STITCH_REGIONS", "INT")
    RETURN_NAMES = ("cropped_image", "cropped_mask", "stitch", "region_count")
    FUNCTION = "crop"
    CATEGORY = "image"
    DESCRIPTION = ("Crop image and mask to one region per connected masked area, all at one working resolution and stacked as "
                   "a batch. Feed the outputs to LanPaint_ImageEncode and the stitch output to LanPaint_DetailerStitchRegions.")

    def crop(self, image, mask, context=1.5, padding=32, target=1024, multiple_of=8, filter="bicubic", min_area=64,
             max_regions=8):
        img, m = _on_device(image, mask)
        labels, n, table = detail.mask_components(m)
        bbox = detail.mask_bbox(m) if n > _cabi.LP_DETAIL_MAX_COMPONENTS else None
        regions = detail.plan_regions((n, table), img.shape[1], img.shape[2], context, padding, multiple_of, target, min_area,
                                      max_regions, bbox=bbox)
        cimg, cmask = detail.crop_regions(img, m, regions, labels, filter)
        stitch = {"original": image, "mask": mask, "regions": regions, "labels": labels.to(mask.device), "filter": filter}
        return (cimg.to(image.device), cmask.to(mask.device), stitch, len(regions))


class LanPaint_DetailerStitchRegions(LanPaint_DetailerStitch):
    """Resample the inpainted regions back and blend them into the original, region after region."""
    STITCH_TYPE, CROP_NODE = "LANPAINT_STITCH_REGIONS", "LanPaint_DetailerCropRegions"
    WINDOWS, CALL = "regions", staticmethod(detail.stitch_regions)
    IMAGE_TIP = "The inpainted regions, at the working resolution, stacked as they were cropped."
    DESCRIPTION = "Stitch the inpainted regions from LanPaint_DetailerCropRegions back into the original image."


NODE_CLASS_MAPPINGS = {"LanPaint_DetailerCropRegions": LanPaint_DetailerCropRegions,
                       "LanPaint_DetailerStitchRegions": LanPaint_DetailerStitchRegions}
NODE_DISPLAY_NAME_MAPPINGS = {"LanPaint_DetailerCropRegions": "LanPaint Detailer Crop (Regions)",
                              "LanPaint_DetailerStitchRegions": "LanPaint Detailer Stitch (Regions)"}
