"""LanPaint_VideoMaskPropagateAnchoredVisible: the video mask propagate that matches every frame against the key frame again and
keeps the mask off whatever passes in front of the subject.

LanPaint_VideoMaskPropagateVisible compares every frame with the key frame's picture through the carried positions; on a long clip
whose subject moves a fraction of a pixel per frame those positions drift, the drift looks like an occluder and the mask is lost.
LanPaint_VideoMaskPropagateAnchored takes that drift out, and puts the mask onto whatever passes in front.  This node
(lanpaint_amd.propagate_anchored_visible, on the HIP device) does both: the anchored re-match, in which a block that does not look
like the key frame even where it fits best counts as covered and takes its correction from its neighbours, and then the visible
node's test and its two outputs on the corrected positions.  It sits where the plain node sits:

    one painted mask + the video -> VideoMaskPropagateAnchoredVisible -> VideoMaskStabilize -> MaskRefine -> ImageEncode / DetailerCrop*

One keyframe only.  A subject that is hidden entirely, or leaves the picture, is lost; occlusion edges are as coarse as the 8 x 8
blocks, which the mask refine sharpens; where the subject stops looking like the key frame it counts as covered.  Host tensors in
and out like the other nodes.  The reference has no such node.  LanPaint_VideoMaskPropagateAnchoredVisibleShots takes the `shots`
of LanPaint_VideoShots and follows the mask inside the key frame's shot only.

This module has its own NODE_CLASS_MAPPINGS: merge them with the others' (INTEGRATION.md section 2(b)).
"""
from __future__ import annotations

from . import propagate_anchored_visible as _both
from ._hostcall import int_in, node_device
from .propagate_nodes import MATCHER_WIDGETS
from .shots_nodes import _PerShot


class LanPaint_VideoMaskPropagateAnchoredVisible:
    """Carry a mask painted on one frame through the video along the picture's motion, re-matched against that frame on every
    frame, and keep it off what passes in front."""

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {
            "image": ("IMAGE", {"tooltip": "The video, one frame per batch entry."}),
            "mask": ("MASK", {"tooltip": "The mask painted on the key frame: one frame, or one per video frame of which only the "
                                         "key frame's is read. Binarised at 0.5. Paint it where the subject is fully in view."}),
            "key_frame": ("INT", {"default": 0, "min": 0, "max": 65534, "step": 1,
                                  "tooltip": "The frame the mask was painted on. The mask is carried forwards and backwards "
                                             "from it, and every frame is matched against and compared with this frame's picture."}),
            **MATCHER_WIDGETS,
            "anchor": ("INT", {"default": _both.DEFAULT_ANCHOR, "min": 0, "max": _both.MAX_ANCHOR, "step": 1,
                               "tooltip": "Pixels searched around the carried position when a frame is matched against the key "
                                          "frame: the largest error one frame can take out, and the drift that is not taken for "
                                          "an occluder. It costs time with its square; 0 switches the correction off."}),
            "occlusion": ("INT", {"default": _both.DEFAULT_OCCLUSION, "min": 0, "max": _both.MAX_OCCLUSION, "step": 1,
                                  "tooltip": "How far, in grey levels averaged over a block, the picture under the mask may differ "
                                             "from the key frame's before the block counts as covered. Lower hides more and starts "
                                             "to mistake noise for an occluder; 0 switches the test off."}),
        }}

    RETURN_TYPES = ("MASK", "MASK")
    RETURN_NAMES = ("mask", "hidden")
    OUTPUT_TOOLTIPS = ("The carried mask without the part that something covers: what the sampler should repaint.",
                       "The part of the subject that is behind something, frame by frame. Add it back to the mask when you want "
                       "to inpaint through the occluder; leave it out to keep the occluder as it is.")
    FUNCTION = "propagate"
    CATEGORY = "mask"
    DESCRIPTION = ("Makes a per-frame video mask from one mask painted on one frame, like the video mask propagate, matches every "
                   "frame against the key frame again, so the mask does not fall behind its subject on a long clip, and keeps it "
                   "off whatever passes in front of the subject: that part moves from `mask` to `hidden`, and comes back when the "
                   "subject does. A block that is covered takes no part in the re-match. Put it in front of the video mask "
                   "stabilize, the mask refine, the encode and the Detailer crops. Not handled: a subject hidden entirely, what "
                   "leaves the picture, occlusion edges finer than a block, several keys, and a subject whose look changes away "
                   "from the key frame.")

    def propagate(self, image, mask, key_frame=0, levels=4, search=2, smooth=8, anchor=_both.DEFAULT_ANCHOR,
                  occlusion=_both.DEFAULT_OCCLUSION):
        int_in(int(anchor), 0, _both.MAX_ANCHOR, "anchor")                   # before anything is moved to the device
        int_in(int(occlusion), 0, _both.MAX_OCCLUSION, "occlusion")
        dev = node_device(image)
        out, hidden = _both.propagate_masks_anchored_visible(image.to(dev), mask.to(dev), int(key_frame), int(levels), int(search),
                                                             int(smooth), int(anchor), int(occlusion))
        return (out.to(mask.device), hidden.to(mask.device))


class LanPaint_VideoMaskPropagateAnchoredVisibleShots(_PerShot, LanPaint_VideoMaskPropagateAnchoredVisible):
    DESCRIPTION = (LanPaint_VideoMaskPropagateAnchoredVisible.DESCRIPTION + " With `shots` the mask is followed inside the key "
                   "frame's shot, and both outputs are empty in every other shot: the subject of one scene is not in the next.")

    def propagate(self, image, mask, key_frame=0, levels=4, search=2, smooth=8, anchor=_both.DEFAULT_ANCHOR,
                  occlusion=_both.DEFAULT_OCCLUSION, shots=None):
        return self._in_key_shot(shots, image, mask, key_frame, levels, search, smooth, anchor, occlusion)


NODE_CLASS_MAPPINGS = {
    "LanPaint_VideoMaskPropagateAnchoredVisible": LanPaint_VideoMaskPropagateAnchoredVisible,
    "LanPaint_VideoMaskPropagateAnchoredVisibleShots": LanPaint_VideoMaskPropagateAnchoredVisibleShots,
}
NODE_DISPLAY_NAME_MAPPINGS = {
    "LanPaint_VideoMaskPropagateAnchoredVisible": "LanPaint Video Mask Propagate (Anchored, Visible)",
    "LanPaint_VideoMaskPropagateAnchoredVisibleShots": "LanPaint Video Mask Propagate (Anchored, Visible, Shots)",
}
