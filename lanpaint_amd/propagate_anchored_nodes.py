"""LanPaint_VideoMaskPropagateAnchored: the video mask propagate that matches every frame against the key frame again.

LanPaint_VideoMaskPropagate carries one painted mask along the picture's motion, one frame-to-frame step after another; on a long
clip whose subject moves a fraction of a pixel per frame the steps' small errors add up and the mask falls behind.  This node
(lanpaint_amd.propagate_anchored, on the HIP device) compares every frame with the key frame's picture carried along the same
motion, block by block under the mask, and moves the carried mask by what that comparison finds, so the error is measured against
the key frame every time and does not add up.  It sits where the plain node sits:

    one painted mask + the video -> VideoMaskPropagateAnchored -> VideoMaskStabilize -> MaskRefine -> ImageEncode / DetailerCrop*

One keyframe only and no occlusion handling.  Where the subject stops looking like the key frame -- it turns, the light changes --
there is nothing to match and the mask drifts as the plain node's does.  Host tensors in and out like the other nodes.  The
reference has no such node.  LanPaint_VideoMaskPropagateAnchoredShots takes the `shots` of LanPaint_VideoShots and follows the
mask inside the key frame's shot only.

This module has its own NODE_CLASS_MAPPINGS: merge them with the others' (INTEGRATION.md section 2(b)).
"""
from __future__ import annotations

from . import propagate_anchored as _anchored
from ._hostcall import int_in, node_device
from .propagate_nodes import MATCHER_WIDGETS
from .shots_nodes import _PerShot


class LanPaint_VideoMaskPropagateAnchored:
    """Carry a mask painted on one frame through the video along the picture's motion, re-matched against that frame on every frame."""

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {
            "image": ("IMAGE", {"tooltip": "The video, one frame per batch entry."}),
            "mask": ("MASK", {"tooltip": "The mask painted on the key frame: one frame, or one per video frame of which only the "
                                         "key frame's is read. Binarised at 0.5."}),
            "key_frame": ("INT", {"default": 0, "min": 0, "max": 65534, "step": 1,
                                  "tooltip": "The frame the mask was painted on. The mask is carried forwards and backwards "
                                             "from it, and every frame is matched against this frame's picture."}),
            **MATCHER_WIDGETS,
            "anchor": ("INT", {"default": _anchored.DEFAULT_ANCHOR, "min": 0, "max": _anchored.MAX_ANCHOR, "step": 1,
                               "tooltip": "Pixels searched around the carried position when a frame is matched against the key "
                                          "frame: the largest error one frame can take out. It costs time with its square; 0 "
                                          "switches the correction off."}),
        }}

    RETURN_TYPES = ("MASK",)
    RETURN_NAMES = ("mask",)
    FUNCTION = "propagate"
    CATEGORY = "mask"
    DESCRIPTION = ("Makes a per-frame video mask from one mask painted on one frame, like the video mask propagate, and matches "
                   "every frame against the key frame again, so the mask does not fall behind its subject on a long clip. Put it "
                   "in front of the video mask stabilize, the mask refine, the encode and the Detailer crops. One keyframe; "
                   "occlusion is not handled, and a subject that stops looking like the key frame drifts as before.")

    def propagate(self, image, mask, key_frame=0, levels=4, search=2, smooth=8, anchor=_anchored.DEFAULT_ANCHOR):
        int_in(int(anchor), 0, _anchored.MAX_ANCHOR, "anchor")               # before anything is moved to the device
        dev = node_device(image)
        out = _anchored.propagate_masks_anchored(image.to(dev), mask.to(dev), int(key_frame), int(levels), int(search), int(smooth),
                                                 int(anchor))
        return (out.to(mask.device),)


class LanPaint_VideoMaskPropagateAnchoredShots(_PerShot, LanPaint_VideoMaskPropagateAnchored):
    DESCRIPTION = (LanPaint_VideoMaskPropagateAnchored.DESCRIPTION + " With `shots` the mask is followed inside the key frame's shot "
                   "and is empty in every other shot: the subject of one scene is not in the next.")

    def propagate(self, image, mask, key_frame=0, levels=4, search=2, smooth=8, anchor=_anchored.DEFAULT_ANCHOR, shots=None):
        return self._in_key_shot(shots, image, mask, key_frame, levels, search, smooth, anchor)


NODE_CLASS_MAPPINGS = {
    "LanPaint_VideoMaskPropagateAnchored": LanPaint_VideoMaskPropagateAnchored,
    "LanPaint_VideoMaskPropagateAnchoredShots": LanPaint_VideoMaskPropagateAnchoredShots,
}
NODE_DISPLAY_NAME_MAPPINGS = {
    "LanPaint_VideoMaskPropagateAnchored": "LanPaint Video Mask Propagate (Anchored)",
    "LanPaint_VideoMaskPropagateAnchoredShots": "LanPaint Video Mask Propagate (Anchored, Shots)",
}
