"""LanPaint_FocusMatch: make the inpainted area as soft as the footage around it.

The decoder draws as sharp as the model can; the shot around the mask is as soft as its lens, motion blur, codec or upscale left it,
and on a soft shot the inpainted area reads as a sticker.  This node measures the edge blur around the mask and under it and blurs
the masked area by the difference (lanpaint_amd.focus.match_focus on the HIP device, the same bits on every run):

    ... -> ImageDecode / DetailerStitch -> (VideoTemporalSmooth) -> FocusMatch -> MultibandBlend -> GrainMatch -> image

Behind the stitch or decode and the temporal smooth, in front of the multiband blend and the grain match: blur removes grain, so grain
goes back after it.  `reference` is the untouched original when there is one; without it the surroundings are read on `image` itself.
Not handled: sharpening (an inpaint softer than its surroundings is left alone), focus that varies across the mask (one blur per
frame or per clip), textures without edges (nothing is measured and nothing happens).  Host tensors in and out like the other nodes.
The reference project has no such node.

This module has its own NODE_CLASS_MAPPINGS: merge them with the others' (INTEGRATION.md section 2(b)).  It stands beside
multiband_nodes.py, whose mappings are fixed.
"""
from __future__ import annotations

from . import _cabi
from . import focus as _focus
from ._hostcall import node_device, node_mask


class LanPaint_FocusMatch:
    """Blur the masked area until its edges are as soft as its surroundings'."""

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {
            "image": ("IMAGE", {"tooltip": "The stitched or decoded result: the picture to correct."}),
            "mask": ("MASK", {"tooltip": "The inpainted area. Measured where it is above 0.5, blurred in proportion to its value."}),
            "strength": ("FLOAT", {"default": 1.0, "min": 0.0, "max": 1.0, "step": 0.0625,
                                   "tooltip": "How much of the measured difference in blur is applied, in sixteenths."}),
            "edge": ("INT", {"default": 8, "min": 1, "max": 255, "step": 1,
                             "tooltip": "Grey levels per pixel, of 255, from which a pixel counts as an edge."}),
            "ring": ("INT", {"default": 2, "min": 1, "max": _cabi.LP_FOCUS_MAX_RING, "step": 1,
                             "tooltip": "How far around the mask the surroundings are read, in tiles of 32 pixels."}),
            "per_frame": ("BOOLEAN", {"default": False,
                                      "tooltip": "Measure every frame on its own instead of the clip as one."}),
        }, "optional": {
            "reference": ("IMAGE", {"tooltip": "Where the surroundings' sharpness is read: the untouched original. Default: image."}),
        }}

    RETURN_TYPES = ("IMAGE",)
    RETURN_NAMES = ("image",)
    FUNCTION = "match"
    CATEGORY = "image/postprocessing"
    DESCRIPTION = ("Soften the inpainted area to the focus of the footage around it. Place it behind the decode or stitch and the "
                   "temporal smooth, in front of LanPaint_MultibandBlend and LanPaint_GrainMatch. It never sharpens, applies one blur "
                   "per frame or clip (no focus gradient across the mask), and leaves areas without edges alone.")

    def match(self, image, mask, strength=1.0, edge=8, ring=2, per_frame=False, reference=None):
        dev = node_device(image)
        ref = None if reference is None else reference.to(dev)
        out = _focus.match_focus(image.to(dev), node_mask(mask, dev), ref, float(strength), int(edge), int(ring), bool(per_frame))
        return (out.to(image.device),)


NODE_CLASS_MAPPINGS = {"LanPaint_FocusMatch": LanPaint_FocusMatch}
NODE_DISPLAY_NAME_MAPPINGS = {"LanPaint_FocusMatch": "LanPaint Focus Match"}
