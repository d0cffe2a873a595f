"""LanPaint_DetailerCropSubjects / LanPaint_DetailerStitchSubjects: the Detailer for several masked subjects that move.

LanPaint_DetailerCropRegions labels the union of the mask over all frames, so one walking person is a smear as wide as their
path and two people whose paths cross are one region; LanPaint_DetailerCropTrack follows the mask with one box per frame, which
spans every subject in it.  These nodes label the mask in space and time on the device, so that a blob and the same blob one
frame later are one component, group the components into at most `max_subjects` subjects, and give every subject a window of
its own that follows it from frame to frame (lanpaint_amd.detail_subjects.plan_subjects).  The sampler gets every (subject,
frame) window at one working size, stacked subject-major: `subject_count` x the clip's length.  Each subject's mask holds its
own components only.  The stitch node puts the subjects back in order and leaves every pixel outside their windows untouched.

    image, mask -> DetailerCropSubjects -> ImageEncode -> sampler -> ImageDecode (no image input) -> DetailerStitchSubjects

With one moving blob the pair equals LanPaint_DetailerCropTrack / LanPaint_DetailerStitchTrack bit for bit.  A colour match
between decode and stitch (LanPaint_DetailerColorMatch) takes `clip_frames` = the clip's length, so that each subject's
stretch of the batch is smoothed as a clip of its own.  Host tensors in and out like the other nodes; the per-pixel work runs
on the HIP device.  The reference has no such node.

This module has its own NODE_CLASS_MAPPINGS: merge them with the others' (INTEGRATION.md section 2(b)).
"""
from __future__ import annotations

from . import _cabi, detail, detail_subjects
from .detail_nodes import LanPaint_DetailerStitch, _on_device
from .detail_track_nodes import LanPaint_DetailerCropTrack


class LanPaint_DetailerCropSubjects:
    """Crop every frame to one window per moving subject of the mask, all windows at one working size, stacked as a batch."""

    @classmethod
    def INPUT_TYPES(s):
        required = dict(LanPaint_DetailerCropTrack.INPUT_TYPES()["required"])
        required["mask"] = ("MASK", {"tooltip": "The inpainting mask (1 = regenerate), one per frame. Its connected areas in "
                                                "space and time become the subjects; each subject's box in a frame steers its "
                                                "window there, and frames it is absent from are bridged."})
        required["min_area"] = ("INT", {"default": 64, "min": 1, "max": 1 << 30, "step": 1,
                                        "tooltip": "Subjects of fewer masked pixels per frame, on average over the frames they "
                                                   "live in, are left out (and stay unchanged)."})
        required["max_subjects"] = ("INT", {"default": 4, "min": 1, "max": _cabi.LP_DETAIL_MAX_REGIONS, "step": 1,
                                            "tooltip": "At most this many subjects; the closest in space and time are merged "
                                                       "beyond it. The sampler's batch is this many times the clip's length."})
        return {"required": required}

    RETURN_TYPES = ("IMAGE", "MASK", "LANPAINT_STITCH_SUBJECTS", "INT")
    RETURN_NAMES = ("cropped_image", "cropped_mask", "stitch", "subject_count")
    FUNCTION = "crop"
    CATEGORY = "image"
    DESCRIPTION = ("Crop every frame of image and mask to one window per moving subject of the mask, all at one working "
                   "resolution and stacked as a batch, subject after subject. Feed the outputs to LanPaint_ImageEncode and the "
                   "stitch output to LanPaint_DetailerStitchSubjects. With LanPaint_DetailerColorMatch in between, set its "
                   "clip_frames to the clip length.")

    def crop(self, image, mask, context=1.5, padding=32, target=1024, multiple_of=8, filter="bicubic", smooth=9, min_area=64,
             max_subjects=4):
        img, m = _on_device(image, mask)
        labels, n, table = detail_subjects.mask_components_frames(detail_subjects._frame_mask(m, img.shape[0], img.shape[1],
                                                                                             img.shape[2]))
        members = detail_subjects.group_subjects((n, table), min_area, min(int(max_subjects), _cabi.LP_DETAIL_MAX_REGIONS))
        if n > _cabi.LP_DETAIL_MAX_COMPONENTS:                      # one subject owns every label: the mask's own boxes
            boxes = (detail.mask_bbox_frames(m),)
        else:
            boxes = detail_subjects.subject_boxes(labels, members)
        subjects = detail_subjects.plan_subjects(members, boxes, img.shape[1], img.shape[2], context, padding, multiple_of,
                                                 target, smooth)
        cimg, cmask = detail_subjects.crop_subjects(img, m, subjects, labels, filter)
        stitch = {"original": image, "mask": mask, "subjects": subjects, "labels": labels.to(mask.device), "filter": filter}
        return (cimg.to(image.device), cmask.to(mask.device), stitch, subjects.subjects)


class LanPaint_DetailerStitchSubjects(LanPaint_DetailerStitch):
    """Resample the inpainted windows back and blend them into the original frames, subject after subject."""
    STITCH_TYPE, CROP_NODE = "LANPAINT_STITCH_SUBJECTS", "LanPaint_DetailerCropSubjects"
    WINDOWS, CALL = "subjects", staticmethod(detail_subjects.stitch_subjects)
    IMAGE_TIP = "The inpainted windows, at the working resolution, stacked as they were cropped."
    DESCRIPTION = "Stitch the inpainted windows from LanPaint_DetailerCropSubjects back into the original frames."


NODE_CLASS_MAPPINGS = {"LanPaint_DetailerCropSubjects": LanPaint_DetailerCropSubjects,
                       "LanPaint_DetailerStitchSubjects": LanPaint_DetailerStitchSubjects}
NODE_DISPLAY_NAME_MAPPINGS = {"LanPaint_DetailerCropSubjects": "LanPaint Detailer Crop (Subjects)",
                              "LanPaint_DetailerStitchSubjects": "LanPaint Detailer Stitch (Subjects)"}
