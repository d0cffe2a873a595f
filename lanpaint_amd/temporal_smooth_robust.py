"""Robust video temporal smooth: a temporal median repairs the frame in which the sampler invented something else.

`temporal_smooth` compares every neighbouring sample with the frame's own pixel.  The one frame in which the sampler put
something else under the mask -- a "pop", the defect a viewer sees first in an inpainted video -- therefore keeps its value, and
the frames next to it lose their whole chain on that side.  This is the second, stricter form beside it, as
`temporal_fill_checked` stands beside `temporal_fill`, and it takes the plain smooth's place:

    decode / stitch -> temporal_smooth_robust -> multiband blend -> grain match

temporal_smooth_robust(images, mask, radius=2, tolerance=24, motion="background", levels=4, search=2, smooth=8)
        -> (out, support, replaced)
        The arguments, the mask, the fields and the walk's positions are those of `temporal_smooth`.  A chain ends only at the
        clip's end or where it leaves the plane, never at a sample that is rejected: the trajectory depends on the fields only.
        Of the up to 2 radius + 1 samples along the motion, the pixel among them, the one with the lower median 8-bit luma (ties
        broken by the walk's order) is the reference; a sample counts while no channel is more than `tolerance` grey levels (of
        255) away from the reference.  Where the pixel itself counts it moves to the binomially weighted mean of itself and what
        counted.  Where it does not and at least two neighbouring samples count -- the reference and one more witness -- it is
        overruled: it becomes their weighted mean.  Else it stays.  `out` fp32 [F, H, W, C]; `support` int32 [F, H, W]: the
        neighbouring samples that counted, 0..2 radius; `replaced` int32 [F, H, W]: 1 where the pixel was overruled, else 0;
        both -1 outside the mask.  Whatever lasts `radius` frames or fewer under the mask is an outlier and is removed on
        purpose; whatever lasts longer stays.  Where nothing is rejected the result is `temporal_smooth`'s bit for bit; so is
        that of a clip of two frames.  One frame or an empty mask returns the images; a still clip is returned bit for bit;
        nothing outside the mask changes.  The fields must fit what lies under the mask: a thing that does not move with
        them cannot be told from a thing invented for a frame (profiles/r35_temporal_smooth_robust.md).
        include/lanpaint_hip.h (lp_tsmooth_robust) states the rule in full.  Not done: a weighted median; a quorum the caller
        sets; motion boundaries finer than a block; a soft mask edge.

HIP tensors only, no CPU fallback, no device -> host read.  The fields, the pyramids, the chunking under
`temporal_smooth.WS_CAP_BYTES` and the checks are `temporal_smooth`'s own code; the gather is one launch for all frames of a
chunk (`robust_frames`).  Nothing is carried from chunk to chunk, so chunking cannot change a bit.
"""
from __future__ import annotations

from . import _cabi
from .temporal_smooth import launch_frames, over_chunks

QUORUM = _cabi.LP_TSMOOTH_ROBUST_QUORUM


def robust_frames(fwd, bwd, known, images, radius=2, tolerance=24, first=0, count=None, fwd_first=0, bwd_first=1, out=None,
                  support=None, replaced=None):
    """The one launch, with the arguments and the checks of `temporal_smooth.smooth_frames` and a third output: the frames
    first .. first + count - 1 of `out`, `support` and `replaced` int32 [F, H, W] are written (new when not given: the other
    frames are then left unwritten).  Returns (out, support, replaced)."""
    return launch_frames("lp_tsmooth_robust", _cabi.LpTsmoothRobustDesc, ((out, "out"), (support, "support"), (replaced, "replaced")),
                          fwd, bwd, known, images, radius, tolerance, first, count, fwd_first, bwd_first)


def temporal_smooth_robust(images, mask, radius=2, tolerance=24, motion="background", levels=4, search=2, smooth=8):
    """What lies under `mask` in the frames `images` [F, H, W, C], pulled towards what agrees with the temporal median along the
    motion, and replaced by it where it is an outlier (module docstring): (out fp32 [F, H, W, C], support int32 [F, H, W],
    replaced int32 [F, H, W]) on the images' device.  No device -> host read."""
    return over_chunks(robust_frames, 2, images, mask, radius, tolerance, motion, levels, search, smooth)
