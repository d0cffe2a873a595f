"""Detailer crop / stitch on the GPU: inpaint at the resolution of the masked region (beyond the reference, whose README lists
"Detailer" as its open item).  Pixel space, once per job, either side of the sampler:

  1. `mask_bbox`      the mask's bounding box on the device (lp_mask_bbox), four integers read back: the job's one device ->
                      host read;
  2. `plan_region`    host integer arithmetic: grow the box by context and padding, snap it to the latent grid, choose the
                      working size;
  3. `crop_resample`  cut the region out of image and mask and resample both to the working size (lp_detail_resample, torch's
                      antialiased bilinear / bicubic from host-built tap tables, `aa_coeffs`);
  4. `stitch`         resample the detailed crop back to the region's size and blend it into the original through the
                      MaskBlend-smoothed mask of the whole image (lp_detail_stitch); outside the region the result is the
                      original bit for bit.

One region serves every frame of the batch (a video is a batch; the sampler needs one shape).  HIP tensors only, no CPU
fallback; results stay on the device.

The region rule, in integers.  `bbox = (r0, r1, c0, c1)` are the inclusive first / last row and column of `mask > 0.5` over
all frames; `r1 < r0` (what lp_mask_bbox returns for an empty mask: (H, -1, W, -1)) raises ValueError.  `context` counts in
thousandths, `c = round(context * 1000) >= 1000`.  Per axis, with image size N, box [a0, a1], `side = a1 - a0 + 1` and
M = multiple_of:
  grow   g = padding + ceil((c - 1000) * side / 2000);  lo = max(a0 - g, 0);  hi = min(a1 + 1 + g, N)       (hi exclusive)
  snap   n = hi - lo,  need = ceil(n / M) * M.  If need <= N the image has room: e = need - n, the low side takes floor(e / 2)
         and the high side the rest (lo -= e // 2; hi = lo + need); a region that now leaves the image is shifted back inside
         (lo < 0: lo = 0; lo + need > N: lo = N - need).  If need > N -- which includes every image smaller than one multiple --
         the region stays as grown and is not a multiple.
  size   target = 0: the working size is the region's own (h, w): no resample.  target > 0: with L = max(h, w), each side s
         becomes  max(1, floor((2 * s * target + L * M) / (2 * L * M))) * M,  i.e. s * target / L rounded to the nearest
         multiple of M, halves up, at least one multiple; the long side becomes `target` when M divides it.
"""
from __future__ import annotations

import ctypes
import dataclasses
import functools
import math

import numpy as np
import torch

from . import _cabi
from ._util import _as_f32c, device_tables, raw_stream
from .videomask import tap_window

FILTERS = ("bilinear", "bicubic")
_SUPPORT = {"bilinear": 1.0, "bicubic": 2.0}          # half-width of the filter: torch's interp_size / 2


@dataclasses.dataclass(frozen=True)
class Region:
    """The window [y0, y0 + h) x [x0, x0 + w) of an H x W image and the working size (oh, ow) it is detailed at."""
    y0: int
    x0: int
    h: int
    w: int
    oh: int
    ow: int
    H: int
    W: int

    @property
    def resampled(self):
        return (self.oh, self.ow) != (self.h, self.w)


def _ceil_div(a, b):
    return -((-a) // b)


def _plan_axis(a0, a1, n_img, c1000, padding, m):
    side = a1 - a0 + 1
    g = padding + _ceil_div((c1000 - 1000) * side, 2000)
    lo, hi = max(a0 - g, 0), min(a1 + 1 + g, n_img)
    need = _ceil_div(hi - lo, m) * m
    if need <= n_img:
        lo -= (need - (hi - lo)) // 2
        lo = min(max(lo, 0), n_img - need)
        hi = lo + need
    return lo, hi - lo


def plan_region(bbox, H, W, context=1.0, padding=0, multiple_of=8, target=0):
    """The module docstring's rule: bbox (r0, r1, c0, c1) inclusive -> Region."""
    r0, r1, c0, c1 = (int(v) for v in bbox)
    H, W, padding, m, target = int(H), int(W), int(padding), int(multiple_of), int(target)
    if H <= 0 or W <= 0:
        raise ValueError(f"image size must be positive, got {H}x{W}")
    if r1 < r0 or c1 < c0:
        raise ValueError("the mask is empty: there is no region to detail")
    if r0 < 0 or c0 < 0 or r1 >= H or c1 >= W:
        raise ValueError(f"bbox {(r0, r1, c0, c1)} lies outside the {H}x{W} image")
    c1000 = int(round(float(context) * 1000))
    if c1000 < 1000:
        raise ValueError(f"context must be >= 1.0, got {context!r}")
    if padding < 0 or m < 1 or target < 0:
        raise ValueError(f"padding >= 0, multiple_of >= 1 and target >= 0 are required, got {padding}, {m}, {target}")
    y0, h = _plan_axis(r0, r1, H, c1000, padding, m)
    x0, w = _plan_axis(c0, c1, W, c1000, padding, m)
    oh, ow = h, w
    if target > 0:
        long_side = max(h, w)
        oh = max(1, (2 * h * target + long_side * m) // (2 * long_side * m)) * m
        ow = max(1, (2 * w * target + long_side * m) // (2 * long_side * m)) * m
    return Region(y0, x0, h, w, oh, ow, H, W)


def _filter_weights(x, filter):
    x = np.abs(x)
    if filter == "bilinear":
        return np.where(x < 1.0, 1.0 - x, 0.0)
    a = -0.5                                              # torch's antialias bicubic (Pillow's), not the a = -0.75 of the plain one
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    far = (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


@functools.lru_cache(maxsize=64)
def aa_coeffs(in_size, out_size, filter="bilinear"):
    """One axis of F.interpolate(mode=filter, align_corners=False, antialias=True) as tables, in fp64: bounds int32
    [out_size, 2] = (first source index, tap count), weights float64 [out_size, ksize], zero past the tap count.  ATen's rule
    (UpSampleKernel.cpp, _compute_indices_min_size_weights_aa): scale = in / out, support = max(scale, 1) * {1, 2}, taps
    int(center -+ support + 0.5) clipped to the source, filter((tap - center + 0.5) / max(scale, 1)), normalised by their sum.
    Cached; the arrays are read-only."""
    if filter not in FILTERS:
        raise ValueError(f"filter must be one of {FILTERS}, got {filter!r}")
    in_size, out_size = int(in_size), int(out_size)
    if in_size <= 0 or out_size <= 0:
        raise ValueError("sizes must be positive")
    scale = float(in_size) / out_size
    support = _SUPPORT[filter] * scale if scale >= 1.0 else _SUPPORT[filter]
    invscale = 1.0 / scale if scale >= 1.0 else 1.0
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    weights = np.zeros((out_size, ksize), np.float64)
    for i in range(out_size):
        center = scale * (i + 0.5)
        xmin, count = tap_window(center, support, in_size)
        w = _filter_weights((np.arange(count, dtype=np.float64) + xmin - center + 0.5) * invscale, filter)
        total = w.sum()
        if total != 0.0:
            w = w / total
        weights[i, :count] = w
        bounds[i] = (xmin, count)
    bounds.flags.writeable = weights.flags.writeable = False
    return bounds, weights


def _hip(t, what):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"lanpaint_amd.detail runs on a HIP device only; no CPU fallback ({what} is not on one)")
    return t


def _mask3(mask):
    if mask.ndim == 2:
        return mask.unsqueeze(0)
    if mask.ndim != 3:
        raise ValueError(f"mask must be [B, H, W], [1, H, W] or [H, W], got {tuple(mask.shape)}")
    return mask


def _check_filter(filter):
    if filter not in FILTERS:
        raise ValueError(f"filter must be one of {FILTERS}, got {filter!r}")


def _check_region(region, H, W):
    if (region.H, region.W) != (H, W):
        raise ValueError(f"the region was planned for a {region.H}x{region.W} image, got {H}x{W}")


def mask_bbox(mask):
    """(row_min, row_max, col_min, col_max), inclusive, of `mask > 0.5` over every frame of a HIP mask [B, H, W], [1, H, W] or
    [H, W]; (H, -1, W, -1) when nothing is set (plan_region raises on it).  Reads four integers back from the device."""
    m = _as_f32c(_mask3(_hip(mask, "mask")))
    planes, h, w = m.shape
    dev = m.device
    box = torch.empty(4, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _cabi.check(_cabi.load().lp_mask_bbox(m.data_ptr(), planes, h, w, box.data_ptr(), raw_stream(dev)), "lp_mask_bbox")
    return tuple(box.cpu().tolist())


def _aa_tables_f32(in_size, out_size, filter):
    """aa_coeffs as the kernel reads it: (bounds int32 [out, 2], weights rounded to float32 [out, ksize])."""
    bounds, weights = aa_coeffs(in_size, out_size, filter)
    return bounds, weights.astype(np.float32)


def _resample(src, y0, x0, h, w, oh, ow, filter):
    """lp_detail_resample on a contiguous fp32 HIP tensor [B, H, W, C]."""
    b, sh, sw, c = src.shape
    dev = src.device
    out = torch.empty((b, oh, ow, c), dtype=torch.float32, device=dev)
    d = _cabi.LpDetailResampleDesc(b, sh, sw, c, y0, x0, h, w, oh, ow, 0, 0)
    d.src, d.dst = src.data_ptr(), out.data_ptr()
    if (oh, ow) != (h, w):
        bx, wx = device_tables(_aa_tables_f32, dev, w, ow, filter)
        by, wy = device_tables(_aa_tables_f32, dev, h, oh, filter)
        d.ksize_x, d.ksize_y = wx.shape[1], wy.shape[1]
        d.bounds_x, d.weights_x, d.bounds_y, d.weights_y = bx.data_ptr(), wx.data_ptr(), by.data_ptr(), wy.data_ptr()
    with torch.cuda.device(dev):
        _cabi.check(_cabi.load().lp_detail_resample(ctypes.byref(d), raw_stream(dev)), "lp_detail_resample")
    return out


def crop_resample(image, mask, region, filter="bilinear"):
    """image [B, H, W, C] and mask ([B, H, W], [1, H, W], [H, W] or None) cut to `region` and resampled to its working size:
    (image [B, oh, ow, C], mask [Bm, oh, ow] or None).  The image takes `filter`, the mask bilinear, and it stays soft."""
    _check_filter(filter)
    img = _as_f32c(_hip(image, "image"))
    if img.ndim != 4:
        raise ValueError(f"image must be [B, H, W, C], got {tuple(image.shape)}")
    _check_region(region, img.shape[1], img.shape[2])
    r = region
    out = _resample(img, r.y0, r.x0, r.h, r.w, r.oh, r.ow, filter)
    if mask is None:
        return out, None
    m = _as_f32c(_mask3(_hip(mask, "mask")))
    if tuple(m.shape[1:]) != (r.H, r.W):
        raise ValueError(f"mask shape {tuple(mask.shape)} does not match images {tuple(image.shape)}")
    return out, _resample(m.unsqueeze(-1), r.y0, r.x0, r.h, r.w, r.oh, r.ow, "bilinear").squeeze(-1)


def stitch(original, detail_img, mask, region, blend_overlap=1, filter="bilinear"):
    """The detailed crop `detail_img` [B, oh, ow, C] back into `original` [B, H, W, C]: resampled to the region's size, blended
    inside the region through MaskBlend's smoothed mask of the whole image (width `blend_overlap`, odd, 1..51), and the
    original bit for bit outside it.  `mask` as for crop_resample: the full-size mask the region was planned from."""
    _check_filter(filter)
    k = blend_overlap
    if not isinstance(k, int) or k < 1 or k > 51 or k % 2 == 0:
        raise ValueError(f"blend_overlap must be an odd integer in [1, 51], got {k!r}")
    orig = _as_f32c(_hip(original, "original"))
    det = _as_f32c(_hip(detail_img, "detail_img").to(orig.device))
    m = _as_f32c(_mask3(_hip(mask, "mask")).to(orig.device))
    if orig.ndim != 4 or det.ndim != 4:
        raise ValueError("original and detail_img must be [B, H, W, C]")
    b, H, W, c = orig.shape
    _check_region(region, H, W)
    r = region
    if tuple(det.shape) != (b, r.oh, r.ow, c):
        raise ValueError(f"detail_img must be {(b, r.oh, r.ow, c)}, got {tuple(det.shape)}")
    if m.shape[0] not in (1, b) or tuple(m.shape[1:]) != (H, W):
        raise ValueError(f"mask shape {tuple(mask.shape)} does not match images {tuple(original.shape)}")
    if r.resampled:
        det = _resample(det, 0, 0, r.oh, r.ow, r.h, r.w, filter)
    dev = orig.device
    out = torch.empty_like(orig)
    d = _cabi.LpDetailStitchDesc(b, H, W, c, r.y0, r.x0, r.h, r.w, k, m.shape[0],
                                 m.data_ptr(), orig.data_ptr(), det.data_ptr(), out.data_ptr())
    with torch.cuda.device(dev):
        _cabi.check(_cabi.load().lp_detail_stitch(ctypes.byref(d), raw_stream(dev)), "lp_detail_stitch")
    return out
