"""Detailer colour match: undo the tone drift a crop picks up between crop and stitch.

A Detailer crop is resampled, VAE-encoded, sampled and VAE-decoded at another resolution; it comes back with a small gain and
offset per channel.  The stitch hides the seam at the mask's edge but not the drift inside the mask, so the detailed area reads
as a patch, and on video the patch flickers.  Outside the mask the decoded crop shows the same content as the original crop, so
statistics taken there compare like with like.  Three steps, all on the device (csrc/color_kernel.hip):

stats   color_stats(detail, reference, mask, margin) -> fp64 [B, 1 + 4 C], row i = {n, then per channel sum d, sum r, sum d^2,
        sum r^2} over the kept pixels of image i.  Pixel (y, x) is kept when every mask element of that image with
        |y' - y| <= margin and |x' - x| <= margin inside the image is <= 0.5 (neighbours outside the image do not count; no
        mask keeps every pixel).  `margin` keeps the statistics away from the band next to the mask, where the decode bleeds.
        Every term is formed and added in fp64; the order of the additions is fixed, so two calls give equal bits.

fit     color_fit(stats, method, strength, smooth, clip_frames) -> fp32 [B, C, 2] = (gain, bias), in fp64 with every operation
        rounded on its own.  With L = clip_frames (0: L = B; L must divide B) and k = smooth (0, or odd 1..129):
          pool      image i is frame f = i % L of clip q = i // L.  P = the sum, in ascending frame order, of the stats rows of
                    frames max(0, f - k // 2) .. min(L - 1, f + k // 2) of clip q; with k = 0, of the whole clip.  The window
                    is cut at the clip's ends, not clamped: no frame is counted twice.
          guard     N = P.n < 64 (LP_COLOR_MIN_COUNT): gain = 1, bias = 0.
          moments   per channel  md = P.d / N, mr = P.r / N, vd = P.dd / N - md * md, vr = P.rr / N - mr * mr.
          gain      "mean": g = 1.  "mean_std": g = 1 when vd <= 1e-8 or vr is not >= 0, otherwise g = sqrt(vr / vd) limited
                    to [0.25, 4].
          bias      b = mr - g * md.
          strength  gain = 1 + s * (g - 1), bias = s * b -- lerp(detail, matched, s) -- both then rounded to fp32.
        For the per-region crop, whose batch is region-major, clip_frames is the number of frames per region, so that pooling
        never crosses regions.

apply   color_apply(detail, coef) -> fp32 [B, H, W, C], out = fl(fl(detail * gain) + bias), unfused.

match() calls them in turn.  HIP tensors only, no CPU fallback; workspace, statistics and coefficients stay on the device, and
nothing is read back to the host.
"""
from __future__ import annotations

import ctypes

import torch

from . import _cabi
from ._hostcall import MAX_BATCH, float_in, image4, int_in, launch, mask_for, require_hip
from ._util import _as_f32c

METHODS = ("mean_std", "mean")
MAX_MARGIN = _cabi.LP_COLOR_MAX_MARGIN


def _check_fit(batch, method, strength, smooth, clip_frames):
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, got {method!r}")
    float_in(strength, 0.0, 1.0, "strength")
    if int_in(smooth, 0, 129, "smooth") and smooth % 2 == 0:
        raise ValueError(f"smooth must be 0 or an odd integer in 1..129, got {smooth!r}")
    if int_in(clip_frames, 0, batch, "clip_frames") and batch % clip_frames:
        raise ValueError(f"clip_frames must be 0 or a divisor of the batch {batch}, got {clip_frames!r}")


def _check_margin(margin):
    int_in(margin, 0, MAX_MARGIN, "margin")


def color_stats(detail, reference, mask=None, margin=8):
    """The masked sums of `detail` and `reference` [B, H, W, C] as fp64 [B, 1 + 4 C] on the device (module docstring).  `mask`
    is [B, H, W], [1, H, W], [H, W] or None (every pixel kept)."""
    _check_margin(margin)
    det = _as_f32c(image4(require_hip(detail, "detail", __name__), "detail", MAX_BATCH))
    ref = _as_f32c(require_hip(reference, "reference", __name__).to(det.device))
    if tuple(ref.shape) != tuple(det.shape):
        raise ValueError(f"reference must be {tuple(det.shape)} like detail, got {tuple(reference.shape)}")
    b, h, w, c = det.shape
    dev = det.device
    m = None if mask is None else mask_for(require_hip(mask, "mask", __name__), b, h, w, dev)
    ws_bytes = _cabi.lp_color_ws_bytes(b, h, w, c)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    stats = torch.empty((b, 1 + 4 * c), dtype=torch.float64, device=dev)
    d = _cabi.LpColorStatsDesc(b, h, w, c, m.shape[0] if m is not None else 1, margin, det.data_ptr(), ref.data_ptr(),
                               m.data_ptr() if m is not None else None, stats.data_ptr(), ws.data_ptr(), ws_bytes)
    launch("lp_color_stats", dev, ctypes.byref(d))
    return stats


def color_fit(stats, method="mean_std", strength=1.0, smooth=1, clip_frames=0):
    """color_stats' table fp64 [B, 1 + 4 C] -> (gain, bias) fp32 [B, C, 2] on the device, by the rule of the module docstring."""
    s = require_hip(stats, "stats", __name__)
    if s.ndim != 2 or s.dtype != torch.float64 or s.shape[0] < 1 or s.shape[1] < 5 or (s.shape[1] - 1) % 4:
        raise ValueError(f"stats must be float64 [B, 1 + 4 C], got {s.dtype} {tuple(s.shape)}")
    b, c = s.shape[0], (s.shape[1] - 1) // 4
    if c > _cabi.LP_DETAIL_MAX_CHANNELS or b > MAX_BATCH:
        raise ValueError(f"stats {tuple(s.shape)}: channels 1..{_cabi.LP_DETAIL_MAX_CHANNELS}, batch 1..{MAX_BATCH}")
    _check_fit(b, method, strength, smooth, clip_frames)
    s = s.contiguous()
    dev = s.device
    coef = torch.empty((b, c, 2), dtype=torch.float32, device=dev)
    kind = _cabi.LP_COLOR_METHOD_MEAN_STD if method == "mean_std" else _cabi.LP_COLOR_METHOD_MEAN
    d = _cabi.LpColorFitDesc(b, c, clip_frames, smooth, kind, 0, float(strength), s.data_ptr(), coef.data_ptr())
    launch("lp_color_fit", dev, ctypes.byref(d))
    return coef


def color_apply(detail, coef, out=None):
    """fl(fl(detail * gain) + bias) per image and channel: detail [B, H, W, C], coef fp32 [B, C, 2].  `out` may be a contiguous
    fp32 tensor of detail's shape on the same device, detail itself included."""
    det = _as_f32c(image4(require_hip(detail, "detail", __name__), "detail", MAX_BATCH))
    b, h, w, c = det.shape
    dev = det.device
    k = require_hip(coef, "coef", __name__)
    if tuple(k.shape) != (b, c, 2) or k.dtype != torch.float32:
        raise ValueError(f"coef must be float32 {(b, c, 2)}, got {k.dtype} {tuple(k.shape)}")
    k = k.to(dev).contiguous()
    if out is None:
        out = torch.empty_like(det)
    elif not torch.is_tensor(out) or out.device != dev or out.dtype != torch.float32 or tuple(out.shape) != tuple(det.shape) \
            or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float32 tensor {tuple(det.shape)} on {dev}")
    d = _cabi.LpColorApplyDesc(b, h, w, c, det.data_ptr(), k.data_ptr(), out.data_ptr())
    launch("lp_color_apply", dev, ctypes.byref(d))
    return out


def match(detail, reference, mask, method="mean_std", strength=1.0, margin=8, smooth=1, clip_frames=0):
    """`detail` [B, H, W, C] with its tone brought to `reference`'s, both measured outside `mask` (module docstring).  Four
    launches on the current stream and no device -> host read."""
    det = image4(require_hip(detail, "detail", __name__), "detail", MAX_BATCH)
    _check_margin(margin)
    _check_fit(det.shape[0], method, strength, smooth, clip_frames)
    det = _as_f32c(det)
    coef = color_fit(color_stats(det, reference, mask, margin), method, strength, smooth, clip_frames)
    return color_apply(det, coef)
