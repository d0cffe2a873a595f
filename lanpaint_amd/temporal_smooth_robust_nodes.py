"""LanPaint_VideoTemporalSmoothRobust: the temporal smooth that also repairs the frame in which the sampler invented something else.

LanPaint_VideoTemporalSmooth compares what the neighbouring frames hold with the frame's own pixel, so a single outlier frame --
the "pop" a viewer sees first in an inpainted video -- keeps its value.  This node (lanpaint_amd.temporal_smooth_robust, on the
HIP device) compares with the temporal median along the motion instead, and where a pixel disagrees with it and two neighbouring
frames stand against the pixel, the pixel is replaced.  It stands where the plain smooth stands, in its place:

    ImageDecode / DetailerStitch* -> VideoTemporalSmoothRobust -> MultibandBlend -> GrainMatch

`radius` is also the longest outlier that is removed: what lasts `radius` frames or fewer under the mask goes, on purpose; what
lasts longer stays.  Host tensors in and out like the other nodes.  The reference has no such node.

LanPaint_VideoTemporalSmoothRobustShots takes the `shots` of LanPaint_VideoShots and works inside every shot on its own.

This module has its own NODE_CLASS_MAPPINGS: merge them with the others' (INTEGRATION.md section 2(b)).
"""
from __future__ import annotations

import torch

from . import temporal_smooth_robust as _robust
from ._hostcall import node_device
from .shots_nodes import _NOTE, _PerShot
from .temporal_smooth_nodes import LanPaint_VideoTemporalSmooth


class LanPaint_VideoTemporalSmoothRobust:
    """Pull the masked area of every video frame towards the temporal median along the motion; replace what is an outlier."""

    @classmethod
    def INPUT_TYPES(s):
        types = {k: dict(v) for k, v in LanPaint_VideoTemporalSmooth.INPUT_TYPES().items()}
        req = types["required"]
        req["radius"] = ("INT", {**req["radius"][1],
                                 "tooltip": "Frames looked at on either side, weighted binomially. Also the longest outlier that is "
                                            "removed: what lasts this many frames or fewer under the mask is replaced."})
        req["tolerance"] = ("INT", {**req["tolerance"][1],
                                    "tooltip": "The most grey levels (of 255) a value may lie away from the temporal median in any "
                                               "channel and still count. A pixel further away than this is an outlier."})
        return types

    RETURN_TYPES = ("IMAGE", "MASK", "MASK")
    RETURN_NAMES = ("image", "support", "replaced")
    FUNCTION = "smooth"
    CATEGORY = "image"
    DESCRIPTION = ("Removes the frame-to-frame boiling of an inpainted video area and repairs outlier frames: every masked pixel "
                   "follows the picture's motion `radius` frames into the past and the future, and the median of what lies there "
                   "is the reference. What agrees with it within `tolerance` is averaged; a pixel that does not, against two "
                   "neighbouring frames that do, is replaced. Use it in place of the plain temporal smooth: behind the decode or "
                   "the Detailer stitch and in front of the multiband blend and the grain match. `radius` is also the longest "
                   "outlier removed: a thing the sampler invented for `radius` frames or fewer under the mask is removed on "
                   "purpose, what lasts longer stays. Choose the `motion` that fits what lies under the mask: what does not move "
                   "with it looks like an outlier. `support` is the share of the neighbouring frames that counted, `replaced` "
                   "is 1 where the pixel was overruled; both are 0 outside the mask.")

    def smooth(self, image, mask, radius=2, tolerance=24, motion="background", levels=4, search=2, smooth=8):
        dev = node_device(image)
        out, support, replaced = _robust.temporal_smooth_robust(image.to(dev), mask.to(dev), int(radius), int(tolerance), motion,
                                                                int(levels), int(search), int(smooth))
        share = torch.clamp(support, min=0).to(torch.float32) / float(2 * int(radius))
        return (out.to(image.device), share.to(mask.device), torch.clamp(replaced, min=0).to(torch.float32).to(mask.device))


class LanPaint_VideoTemporalSmoothRobustShots(_PerShot, LanPaint_VideoTemporalSmoothRobust):
    DESCRIPTION = LanPaint_VideoTemporalSmoothRobust.DESCRIPTION + _NOTE

    def smooth(self, image, mask, radius=2, tolerance=24, motion="background", levels=4, search=2, smooth=8, shots=None):
        return self._per_shot(shots, {"image": image, "mask": mask}, radius=radius, tolerance=tolerance, motion=motion, levels=levels,
                              search=search, smooth=smooth)


NODE_CLASS_MAPPINGS = {
    "LanPaint_VideoTemporalSmoothRobust": LanPaint_VideoTemporalSmoothRobust,
    "LanPaint_VideoTemporalSmoothRobustShots": LanPaint_VideoTemporalSmoothRobustShots,
}
NODE_DISPLAY_NAME_MAPPINGS = {
    "LanPaint_VideoTemporalSmoothRobust": "LanPaint Video Temporal Smooth (Robust)",
    "LanPaint_VideoTemporalSmoothRobustShots": "LanPaint Video Temporal Smooth (Robust, Shots)",
}
