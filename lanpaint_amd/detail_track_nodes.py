"""LanPaint_DetailerCropTrack / LanPaint_DetailerStitchTrack: the Detailer with a window that follows a moving mask.

LanPaint_DetailerCrop takes the bounding box of the mask over all frames, so a small subject that crosses the frame of a video
gives a region that is most of the frame.  These nodes find one bounding box per frame on the device, plan one window size for
the clip and a path of window origins smoothed over `smooth` frames (lanpaint_amd.detail.plan_track), and hand the sampler
every frame's own window at one working size: the batch keeps its length and its shape.  However strong the smoothing, a
frame's mask stays inside its window.  The stitch node puts every frame's crop back where it was cut and leaves every pixel
outside that frame's window untouched.

    image, mask -> DetailerCropTrack -> ImageEncode -> sampler -> ImageDecode (no image input) -> DetailerStitchTrack

With a mask that stands still the pair equals LanPaint_DetailerCrop / LanPaint_DetailerStitch on a window of the same place
and size.  Host tensors in and out like the other nodes; the per-pixel work runs on the HIP device.  The reference has no such
node.

This module has its own NODE_CLASS_MAPPINGS: merge them with the others' (INTEGRATION.md section 2(b)).
"""
from __future__ import annotations

from . import detail
from .detail_nodes import LanPaint_DetailerCrop, LanPaint_DetailerStitch, _on_device


class LanPaint_DetailerCropTrack:
    """Crop every frame of image and mask to a window of one size that follows the mask, at one working size."""

    @classmethod
    def INPUT_TYPES(s):
        required = dict(LanPaint_DetailerCrop.INPUT_TYPES()["required"])
        required["mask"] = ("MASK", {"tooltip": "The inpainting mask (1 = regenerate), one per frame. Each frame's bounding box "
                                                "steers that frame's window; frames with an empty mask are bridged."})
        required["smooth"] = ("INT", {"default": 9, "min": 1, "max": 129, "step": 2,
                                      "tooltip": "Number of frames the window's path is averaged over (odd; 1 = follow the "
                                                 "mask frame by frame)."})
        return {"required": required}

    RETURN_TYPES = ("IMAGE", "MASK", "LANPAINT_STITCH_TRACK")
    RETURN_NAMES = ("cropped_image", "cropped_mask", "stitch")
    FUNCTION = "crop"
    CATEGORY = "image"
    DESCRIPTION = ("Crop every frame of image and mask to a window that follows the mask through the video, all at one working "
                   "resolution. Feed the outputs to LanPaint_ImageEncode and the stitch output to LanPaint_DetailerStitchTrack.")

    def crop(self, image, mask, context=1.5, padding=32, target=1024, multiple_of=8, filter="bicubic", smooth=9):
        img, m = _on_device(image, mask)
        track = detail.plan_track(detail.mask_bbox_frames(m), img.shape[1], img.shape[2], context, padding, multiple_of, target,
                                  smooth, frames=img.shape[0])
        cimg, cmask = detail.crop_track(img, m, track, filter)
        stitch = {"original": image, "mask": mask, "track": track, "filter": filter}
        return (cimg.to(image.device), cmask.to(mask.device), stitch)


class LanPaint_DetailerStitchTrack(LanPaint_DetailerStitch):
    """Resample every frame's inpainted window back and blend it into the original where it was cut."""
    STITCH_TYPE, CROP_NODE = "LANPAINT_STITCH_TRACK", "LanPaint_DetailerCropTrack"
    WINDOWS, CALL = "track", staticmethod(detail.stitch_track)
    IMAGE_TIP = "The inpainted windows, at the working resolution, one per frame."
    DESCRIPTION = "Stitch the inpainted windows from LanPaint_DetailerCropTrack back into the original frames."


NODE_CLASS_MAPPINGS = {"LanPaint_DetailerCropTrack": LanPaint_DetailerCropTrack,
                       "LanPaint_DetailerStitchTrack": LanPaint_DetailerStitchTrack}
NODE_DISPLAY_NAME_MAPPINGS = {"LanPaint_DetailerCropTrack": "LanPaint Detailer Crop (Track)",
                              "LanPaint_DetailerStitchTrack": "LanPaint Detailer Stitch (Track)"}
