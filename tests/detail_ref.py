"""Shared arbiters of the Detailer tests (tests/test_detail_host.py, tests/test_gpu_detail.py): torch's CPU operators in fp64
and the bound the fp32 resample is held to.  Nothing here touches a device."""
import numpy as np
import torch
import torch.nn.functional as F

from lanpaint_amd import detail
from lanpaint_amd.blend import gaussian_kernel_2d


def ref64(x, size, filter):
    """x [B, h, w, C] (any float dtype, CPU) -> float64 [B, oh, ow, C]: the definition of crop-resample."""
    if tuple(x.shape[1:3]) == tuple(size):
        return x.double()
    return F.interpolate(x.movedim(-1, 1).double(), size=tuple(size), mode=filter, align_corners=False,
                         antialias=True).movedim(1, -1).contiguous()


def dense(bounds, weights, in_size):
    """The tap table as an [out, in] matrix."""
    a = np.zeros((bounds.shape[0], in_size), weights.dtype)
    for i, (first, count) in enumerate(bounds):
        a[i, first:first + count] = weights[i, :count]
    return a


def apply_tables64(x, size, filter):
    """x float64 numpy [h, w] through detail.aa_coeffs' fp64 tables: rows then columns."""
    h, w = x.shape
    by, wy = detail.aa_coeffs(h, size[0], filter)
    bx, wx = detail.aa_coeffs(w, size[1], filter)
    return dense(by, wy, h) @ (x @ dense(bx, wx, w).T)


def apply_tables32(x, size, filter):
    """What lp_detail_resample computes, restated with numpy: fp32-rounded weights, horizontal pass then vertical, every
    product and partial sum rounded to fp32, taps ascending (the device may fuse a product into its sum: one rounding less)."""
    h, w = x.shape
    by, wy = detail.aa_coeffs(h, size[0], filter)
    bx, wx = detail.aa_coeffs(w, size[1], filter)
    wy, wx = wy.astype(np.float32), wx.astype(np.float32)
    x = x.astype(np.float32)
    mid = np.zeros((h, size[1]), np.float32)
    for t in range(wx.shape[1]):
        idx = np.minimum(bx[:, 0] + t, w - 1)
        mid += x[:, idx] * np.where(t < bx[:, 1], wx[:, t], np.float32(0))[None, :]
    out = np.zeros((size[0], size[1]), np.float32)
    for t in range(wy.shape[1]):
        idx = np.minimum(by[:, 0] + t, h - 1)
        out += mid[idx, :] * np.where(t < by[:, 1], wy[:, t], np.float32(0))[:, None]
    return out


def bound(in_hw, out_hw, filter, xmax):
    """b = (taps_x + taps_y + 2) * 2^-23 * L * max|x|: taps_* the two tables' ksize, L the product of their largest sum of
    |w|.  The worst case of fp32-rounded weights plus two fp32 sums; derived from the tables, not tuned.  0 for an identity."""
    if tuple(in_hw) == tuple(out_hw):
        return 0.0
    _, wy = detail.aa_coeffs(in_hw[0], out_hw[0], filter)
    _, wx = detail.aa_coeffs(in_hw[1], out_hw[1], filter)
    big = float(np.abs(wy).sum(1).max() * np.abs(wx).sum(1).max())
    return (wx.shape[1] + wy.shape[1] + 2) * 2.0 ** -23 * big * float(xmax)


def smooth_mask_ref(mask, k):
    """mask [Bm, H, W] fp32 CPU -> MaskBlend's smoothed mask, torch ops (section 1 of the Detailer contract)."""
    m = mask.float().unsqueeze(1)
    m = F.max_pool2d(m, kernel_size=k, stride=1, padding=k // 2)
    return F.conv2d(m, gaussian_kernel_2d(k).view(1, 1, k, k), padding=k // 2)[:, 0]


def stitch_ref(original, detail_img, mask, region, k, filter):
    """The stitch restated with torch CPU ops: fp64 resample rounded to fp32, unfused fp32 lerp inside the region."""
    r = region
    m = smooth_mask_ref(mask if mask.ndim == 3 else mask.unsqueeze(0), k)[:, r.y0:r.y0 + r.h, r.x0:r.x0 + r.w].unsqueeze(-1)
    d = ref64(detail_img, (r.h, r.w), filter).float()
    out = original.clone()
    o = original[:, r.y0:r.y0 + r.h, r.x0:r.x0 + r.w, :]
    out[:, r.y0:r.y0 + r.h, r.x0:r.x0 + r.w, :] = o * (1.0 - m) + d * m
    return out
