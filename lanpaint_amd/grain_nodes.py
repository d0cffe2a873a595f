"""LanPaint_GrainMatch: put the grain back that an inpainted area lacks.

A photograph or a video frame carries sensor noise, film grain or compression noise; what the VAE decoder returns under the mask
is clean.  On a still the area reads as too smooth, on video as a patch that sits still while the grain around it moves.  This
node measures the grain outside the mask (or on a reference image), measures what is left of it inside, and adds a synthesized
grain of the missing amount under the mask (lanpaint_amd.grain, on the HIP device).  It goes last in the chain:

    ... -> DetailerColorMatch -> Stitch* / MaskBlend -> MultibandBlend -> GrainMatch

Host tensors in and out like the other nodes.  The reference has no such node.

This module has its own NODE_CLASS_MAPPINGS: merge them with the others' (INTEGRATION.md section 2(b)).
"""
from __future__ import annotations

from . import grain as _grain
from ._hostcall import node_device, node_mask

GRAIN_SIZES = ("auto", "fine", "medium", "coarse")


class LanPaint_GrainMatch:
    """Measure the grain around the mask and add what is missing under it."""

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {
            "image": ("IMAGE", {"tooltip": "The finished image or video frames, after the stitch and the blend: the area under "
                                           "the mask is clean, the rest carries the original's grain."}),
            "mask": ("MASK", {"tooltip": "Where the image was inpainted. The grain is added in proportion to the mask; pixels "
                                         "with mask 0 keep their bits."}),
            "strength": ("FLOAT", {"default": 1.0, "min": 0.0, "max": 2.0, "step": 0.05,
                                   "tooltip": "Scales the fitted grain amplitude: 1 matches the measured grain, 0 returns the "
                                              "image unchanged."}),
            "grain_size": (list(GRAIN_SIZES), {"default": "auto",
                                               "tooltip": "fine is white noise, medium a 3 x 3 and coarse a 5 x 5 binomial grain; "
                                                          "auto picks the size from the measured spectrum."}),
            "monochrome": ("BOOLEAN", {"default": False,
                                       "tooltip": "One grain for all channels (luminance grain) instead of one per channel."}),
            "flat": ("INT", {"default": 64, "min": 0, "max": 255, "step": 1,
                             "tooltip": "Texture reject: a pixel is measured only when its 5 x 5 neighbourhood spans at most this "
                                        "many 8-bit codes. 255 measures everything."}),
            "margin": ("INT", {"default": 8, "min": 0, "max": 25, "step": 1,
                               "tooltip": "Pixels to stay away from the mask when measuring the grain outside it. Unused with a "
                                          "reference image."}),
            "seed": ("INT", {"default": 0, "min": 0, "max": 0xffffffffffffffff,
                             "tooltip": "Seed of the grain. Every frame of a batch gets its own grain from it."}),
            "clip_frames": ("INT", {"default": 0, "min": 0, "max": 65535, "step": 1,
                                    "tooltip": "Frames per clip when the batch holds several clips: the grain is fitted per clip. "
                                               "0 fits the whole batch as one clip; otherwise it must divide the batch."}),
        }, "optional": {
            "reference": ("IMAGE", {"tooltip": "Measure the grain here instead of outside the mask: the untouched original or a "
                                               "grain plate, any size and frame count, the same channel count."}),
        }}

    RETURN_TYPES = ("IMAGE",)
    RETURN_NAMES = ("image",)
    FUNCTION = "match"
    CATEGORY = "image/postprocessing"
    DESCRIPTION = ("Puts back the grain an inpainted area lacks: measures sensor noise, film grain or compression noise outside "
                   "the mask (or on a reference image) and adds a synthesized grain of the missing amount under the mask. Put it "
                   "last, behind the stitch and the multiband blend; on video every frame gets its own grain.")

    def match(self, image, mask, strength=1.0, grain_size="auto", monochrome=False, flat=64, margin=8, seed=0, clip_frames=0,
              reference=None):
        dev = node_device(image)
        ref = None if reference is None else reference.to(dev)
        out = _grain.match(image.to(dev), node_mask(mask, dev), ref, float(strength), str(grain_size), bool(monochrome), int(flat),
                           int(margin), int(seed), int(clip_frames))
        return (out.to(image.device),)


NODE_CLASS_MAPPINGS = {"LanPaint_GrainMatch": LanPaint_GrainMatch}
NODE_DISPLAY_NAME_MAPPINGS = {"LanPaint_GrainMatch": "LanPaint Grain Match"}
