"""LanPaint_VideoMaskPropagateVisible: the video mask propagate that keeps the mask off whatever passes in front of the subject.

LanPaint_VideoMaskPropagate carries one painted mask along the picture's motion; when the subject passes behind a lamp post the
carried mask lies on the post, and the sampler repaints the post.  This node (lanpaint_amd.propagate_visible, on the HIP device)
compares every frame with the key frame's picture carried along the same motion, block by block under the mask, takes the part
that no longer looks like the subject out of the mask and returns it as a second output.  It sits where the plain node sits:

    one painted mask + the video -> VideoMaskPropagateVisible -> VideoMaskStabilize -> MaskRefine -> ImageEncode / DetailerCrop*

One keyframe only.  A subject that is hidden entirely, or leaves the picture, is lost; occlusion edges are as coarse as the 8 x 8
blocks, which the mask refine sharpens.  Host tensors in and out like the other nodes.  The reference has no such node.

This module has its own NODE_CLASS_MAPPINGS: merge them with the others' (INTEGRATION.md section 2(b)).
"""
from __future__ import annotations

from . import propagate_visible as _visible
from ._hostcall import node_device
from .propagate_nodes import MATCHER_WIDGETS


class LanPaint_VideoMaskPropagateVisible:
    """Carry a mask painted on one frame through the video along the picture's motion, and keep it off what passes in front."""

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {
            "image": ("IMAGE", {"tooltip": "The video, one frame per batch entry."}),
            "mask": ("MASK", {"tooltip": "The mask painted on the key frame: one frame, or one per video frame of which only the "
                                         "key frame's is read. Binarised at 0.5. Paint it where the subject is fully in view."}),
            "key_frame": ("INT", {"default": 0, "min": 0, "max": 65534, "step": 1,
                                  "tooltip": "The frame the mask was painted on. The mask is carried forwards and backwards "
                                             "from it, and every frame is compared with this frame's picture."}),
            **MATCHER_WIDGETS,
            "occlusion": ("INT", {"default": _visible.DEFAULT_OCCLUSION, "min": 0, "max": _visible.MAX_OCCLUSION, "step": 1,
                                  "tooltip": "How far, in grey levels averaged over a block, the picture under the mask may differ "
                                             "from the key frame's before the block counts as covered. Lower hides more and starts "
                                             "to mistake noise and fine motion for an occluder; 0 switches the test off."}),
        }}

    RETURN_TYPES = ("MASK", "MASK")
    RETURN_NAMES = ("mask", "hidden")
    OUTPUT_TOOLTIPS = ("The carried mask without the part that something covers: what the sampler should repaint.",
                       "The part of the subject that is behind something, frame by frame. Add it back to the mask when you want "
                       "to inpaint through the occluder; leave it out to keep the occluder as it is.")
    FUNCTION = "propagate"
    CATEGORY = "mask"
    DESCRIPTION = ("Makes a per-frame video mask from one mask painted on one frame, like the video mask propagate, and keeps it "
                   "off whatever passes in front of the subject: where the picture under the carried mask stops looking like the "
                   "key frame, that part moves from `mask` to `hidden`, and comes back when the subject does. Put it in front of "
                   "the video mask stabilize, the mask refine, the encode and the Detailer crops. One keyframe; a subject that is "
                   "covered entirely or leaves the picture is lost.")

    def propagate(self, image, mask, key_frame=0, levels=4, search=2, smooth=8, occlusion=_visible.DEFAULT_OCCLUSION):
        dev = node_device(image)
        out, hidden = _visible.propagate_masks_visible(image.to(dev), mask.to(dev), int(key_frame), int(levels), int(search),
                                                       int(smooth), int(occlusion))
        return (out.to(mask.device), hidden.to(mask.device))


NODE_CLASS_MAPPINGS = {"LanPaint_VideoMaskPropagateVisible": LanPaint_VideoMaskPropagateVisible}
NODE_DISPLAY_NAME_MAPPINGS = {"LanPaint_VideoMaskPropagateVisible": "LanPaint Video Mask Propagate (Visible)"}
