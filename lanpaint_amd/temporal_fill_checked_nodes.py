"""LanPaint_VideoTemporalFillChecked: the video temporal fill with a consistency check on what it borrows.

LanPaint_VideoTemporalFill takes every masked pixel from the nearest frame that shows it, along the background's motion, and
believes that motion everywhere.  When something other than the masked subject moves through the hole -- a second object, a
shadow -- it pastes the wrong picture, the encode takes it as known, and the sampler never repaints it.  This node
(lanpaint_amd.temporal_fill_checked, on the HIP device) asks two witnesses: the nearest earlier frame and the nearest later
frame.  Where both show a pixel and, over a block of 8 x 8 pixels, do not show the same thing, the block is disputed and is left
in `remaining` for the sampler.  It stands where the plain node stands:

    mask chain -> VideoTemporalFillChecked -> (remaining mask) MaskFill -> ImageEncode / DetailerCrop*

Borrowed pixels are not colour-matched (DetailerColorMatch exists).  Host tensors in and out like the other nodes.  The reference
has no such node.

This module has its own NODE_CLASS_MAPPINGS: merge them with the others' (INTEGRATION.md section 2(b)).
"""
from __future__ import annotations

import torch

from . import temporal_fill_checked as _checked
from ._hostcall import node_device
from .temporal_fill_nodes import LanPaint_VideoTemporalFill


class LanPaint_VideoTemporalFillChecked:
    """Fill the masked area of every video frame from other frames, keeping only what an earlier and a later frame agree on."""

    @classmethod
    def INPUT_TYPES(s):
        required = dict(LanPaint_VideoTemporalFill.INPUT_TYPES()["required"])
        required["agree"] = ("INT", {"default": 8, "min": 1, "max": 255, "step": 1,
                                     "tooltip": "How far the earlier and the later frame may differ over a block of 8 x 8 pixels "
                                                "before it is disputed: the mean difference in grey levels (of 255), a brightness "
                                                "shift forgiven. Lower disputes more and leaves more to the sampler."})
        return {"required": required}

    RETURN_TYPES = ("IMAGE", "MASK", "MASK", "MASK")
    RETURN_NAMES = ("image", "remaining", "filled", "verified")
    FUNCTION = "fill"
    CATEGORY = "image"
    DESCRIPTION = ("Fills the masked area of a video from its other frames, like the video temporal fill, and checks what it "
                   "borrows: where an earlier and a later frame both show a masked pixel, the two are compared block by block. A "
                   "dispute is a block in which they disagree by more than `agree` grey levels on average, as when a second object "
                   "passes behind the subject; it is not filled and stays in `remaining`. Give `remaining` to the mask fill, the "
                   "encode and the Detailer crops as the mask. `verified` marks the pixels two frames agreed on; the other filled "
                   "pixels rest on one frame alone. Borrowed pixels are not colour-matched.")

    def fill(self, image, mask, levels=4, search=2, smooth=8, reach=0, agree=8):
        dev = node_device(image)
        filled, remaining, source, witnesses = _checked.temporal_fill_checked(image.to(dev), mask.to(dev), int(levels), int(search),
                                                                              int(smooth), int(reach), int(agree))
        frames = torch.arange(source.shape[0], dtype=torch.int32, device=dev).view(-1, 1, 1)
        borrowed = ((source >= 0) & (source != frames)).to(torch.float32)          # the mask's bits without `remaining`
        verified = (witnesses == 2).to(torch.float32)
        return (filled.to(image.device), remaining.to(mask.device), borrowed.to(mask.device), verified.to(mask.device))


NODE_CLASS_MAPPINGS = {"LanPaint_VideoTemporalFillChecked": LanPaint_VideoTemporalFillChecked}
NODE_DISPLAY_NAME_MAPPINGS = {"LanPaint_VideoTemporalFillChecked": "LanPaint Video Temporal Fill (Checked)"}
