"""Video mask stabilize: a temporal median and a binomial smoothing of a per-frame mask's signed distance field.

A per-frame mask that comes from a segmenter, or was painted frame by frame, flickers: its edge jitters by a pixel or two from
frame to frame, and single frames come back empty or carry a stray blob.  Everything downstream inherits that -- the latent mask
changes shape every frame, the Detailer windows jump, the stitch seam crawls.  `LanPaint_MaskRefine` treats every frame on its
own and `LanPaint_VideoMaskEditor` only morphs between painted keyframes; this is the mask's own smoothing in time.  Use it
behind a per-frame segmenter or the video mask editor and in front of the mask refine, the encode and the Detailer crops.

stabilize_masks(mask, median=1, smooth=2, grow=0.0, feather=0.0) -> mask [F, H, W]
        every frame is binarised at 0.5 and gets its exact signed squared Euclidean distance (videomask.keyframe_edt); along time,
        per pixel, the median of the 2 median + 1 neighbouring frames' values (end frames replicated) removes a dropout or a stray
        blob that lasts at most `median` frames; the distance, capped at 64 pixels, is then smoothed with the binomial weights of
        radius `smooth`, which calms an edge that jitters.  The smoothing alone does not repair a dropped frame: that is the
        median's work.  `grow` (pixels, |grow| <= 256) moves the edge outwards, `feather` (pixels, 0..64) replaces the hard
        threshold by a ramp of that half-width.  The arithmetic is exact integers, then fp64 in a fixed order, so the result is the
        same bits on every run: at grow = 0 an all-zero video stays exactly 0, an all-one video exactly 1, and a video whose frames
        are all equal comes back binarised.  include/lanpaint_hip.h (lp_mask_stabilize) states the rule in full.

HIP tensors only, no CPU fallback.  The distances are computed in chunks of frames whose buffers stay under WS_CAP_BYTES and
folded into one int32 [F, H, W]; frames are independent there, so chunking cannot change a bit.  Then one launch runs along time.
"""
from __future__ import annotations

import ctypes

import torch

from . import _cabi, videomask
from ._hostcall import float_in, int_in, launch, require_hip
from ._util import _as_f32c

MAX_SIDE = _cabi.LP_VMASK_MAX_SIDE
MAX_MEDIAN = _cabi.LP_STAB_MAX_MEDIAN
MAX_SMOOTH = _cabi.LP_STAB_MAX_SMOOTH
MAX_GROW = _cabi.LP_STAB_MAX_GROW
MAX_FEATHER = _cabi.LP_STAB_MAX_FEATHER
WS_CAP_BYTES = 1 << 30


def signed_d2(mask):
    """Stage 1 for `mask` fp32 [F, H, W] on a HIP device: int32 [F, H, W], +d2 to the nearest background pixel on the foreground
    (v >= 0.5), -d2 to the nearest foreground pixel on the background, +-LP_STAB_Q_FAR on a full or an empty frame.  The frames
    go through videomask.edt_chunks under WS_CAP_BYTES; one lp_mask_signed_d2 launch per chunk."""
    F, H, W = mask.shape
    q = torch.empty((F, H, W), dtype=torch.int32, device=mask.device)
    for s, n, d2 in videomask.edt_chunks(mask, WS_CAP_BYTES):
        launch("lp_mask_signed_d2", mask.device, d2.data_ptr(), n, H, W, q[s:s + n].data_ptr())
    return q


def stabilize_q(q, median=1, smooth=2, grow=0.0, feather=0.0):
    """Stages 2 to 5 on the signed squared distances `q` int32 [F, H, W] (from `signed_d2`): fp32 [F, H, W].  One launch."""
    int_in(median, 0, MAX_MEDIAN, "median")
    int_in(smooth, 0, MAX_SMOOTH, "smooth")
    grow = float_in(grow, -MAX_GROW, MAX_GROW, "grow")
    feather = float_in(feather, 0, MAX_FEATHER, "feather")
    require_hip(q, "q", __name__)
    if q.dtype != torch.int32 or q.ndim != 3 or not q.is_contiguous():
        raise ValueError("q must be a contiguous int32 [F, H, W]")
    F, H, W = q.shape
    out = torch.empty((F, H, W), dtype=torch.float32, device=q.device)
    d = _cabi.LpStabilizeDesc(F, H, W, median, smooth, 0, grow, feather, q.data_ptr(), out.data_ptr())
    launch("lp_mask_stabilize", q.device, ctypes.byref(d))
    return out


def stabilize_masks(mask, median=1, smooth=2, grow=0.0, feather=0.0):
    """`mask` [F, H, W] (or one frame [H, W]) stabilized along time (module docstring); fp32 [F, H, W] back, on the mask's
    device.  The EDT's launches per chunk of frames, one fold per chunk, one temporal launch; no device -> host read."""
    int_in(median, 0, MAX_MEDIAN, "median")
    int_in(smooth, 0, MAX_SMOOTH, "smooth")
    float_in(grow, -MAX_GROW, MAX_GROW, "grow")
    float_in(feather, 0, MAX_FEATHER, "feather")
    require_hip(mask, "mask", __name__)
    if mask.ndim == 2:
        mask = mask.unsqueeze(0)
    if mask.ndim != 3:
        raise ValueError(f"mask must be [F, H, W] or [H, W], got {tuple(mask.shape)}")
    F, H, W = mask.shape
    if F < 1 or min(H, W) < 1 or max(H, W) > MAX_SIDE:
        raise ValueError(f"mask {tuple(mask.shape)}: sides 1..{MAX_SIDE}, at least one frame")
    return stabilize_q(signed_d2(_as_f32c(mask)), median, smooth, grow, feather)
