"""Shared arbiters of the Detailer tests (tests/test_detail_host.py, tests/test_gpu_detail.py, tests/test_gpu_detail_shapes.py):
torch's CPU operators in fp64, the bound the fp32 resample is held to, and the exact response to a single non-zero element.
Nothing here touches a device."""
import numpy as np
import torch
import torch.nn.functional as F

from lanpaint_amd import detail
from lanpaint_amd.blend import gaussian_kernel_2d


# (window) -> (output) size pairs of tests/test_gpu_detail_shapes.py, by family; the host tests pin the tables of every one.
TILE_OH = (15, 16, 17, 33)                       # around lp_detail_resample's 16-row tile, and a third tile
SHAPE_PAIRS = {
    "degenerate": [((1, 1), (7, 9)), ((9, 7), (1, 1)), ((1, 300), (1, 77)), ((300, 1), (77, 1))],
    "long_taps": [((2000, 40), (50, 40)), ((40, 4096), (40, 33)), ((1100, 24), (16, 24))],
    "side_limit": [((3, 5), (3, 32768)), ((5, 3), (32768, 3))],
    "tile_c1": [((37, 41), (oh, ow)) for oh in TILE_OH for ow in (252, 255, 256, 257, 260)],      # rowE = ow
    "tile_c3": [((37, 41), (oh, ow)) for oh in TILE_OH for ow in (84, 85, 86, 87)],               # rowE = 252 / 255 / 258 / 261
    "channels": [((23, 31), (40, 19)), ((40, 19), (23, 31))],
}
ALL_PAIRS = [pair for family in SHAPE_PAIRS.values() for pair in family]
IMPULSE = 0.7310586


def torch_aa(x, size, filter):
    """F.interpolate(x [B, C, h, w], size, mode=filter, align_corners=False, antialias=True) on the CPU, in x's dtype.
    A width of 1 kept at 1 is asked of torch as a width of 2 kept at 2 (the column twice, column 0 taken): the operator is
    separable, an axis kept at its size is the identity, and torch's CPU kernel answers such a one-column image with one
    value for the whole column ((300, 1) -> (77, 1), torch 2.10), which no separable operator does."""
    if x.shape[-1] == 1 and size[1] == 1 and x.shape[-2] != size[0]:
        wide = F.interpolate(x.expand(-1, -1, -1, 2).contiguous(), size=(size[0], 2), mode=filter, align_corners=False,
                             antialias=True)
        assert torch.equal(wide[..., 0], wide[..., 1])
        return wide[..., :1].contiguous()
    return F.interpolate(x, size=tuple(size), mode=filter, align_corners=False, antialias=True)


def ref64(x, size, filter):
    """x [B, h, w, C] (any float dtype, CPU) -> float64 [B, oh, ow, C]: the definition of crop-resample."""
    if tuple(x.shape[1:3]) == tuple(size):
        return x.double()
    return torch_aa(x.movedim(-1, 1).double(), size, filter).movedim(1, -1).contiguous()


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


def tables32(in_size, out_size, filter):
    """One axis as the kernel reads it: (bounds, the dense [out, in] matrix of the fp32-rounded weights)."""
    bounds, weights = detail.aa_coeffs(in_size, out_size, filter)
    return bounds, dense(bounds, weights.astype(np.float32), in_size)


def impulse_ref(in_hw, out_hw, filter, at, value=IMPULSE):
    """The resample of an in_hw image that is zero except `value` at `at` = (sy, sx): float32 [oh, ow] =
    fl32(wy32[:, sy] (x) fl32(value * wx32[:, sx])).  Every other product of either pass is an exact zero and
    fma(p, w, 0) = fl(p * w), so a kernel that reads the tables rightly gives this with one rounding per pass whatever its tap
    order and whether or not its multiply-add fuses: equal as values, a zero of either sign being zero.  No non-zero value on
    the way may be subnormal, so that a flushed denormal cannot pass for an indexing error."""
    sy, sx = at
    _, ay = tables32(in_hw[0], out_hw[0], filter)
    _, ax = tables32(in_hw[1], out_hw[1], filter)
    mid = np.float32(value) * ax[:, sx]
    out = ay[:, sy][:, None] * mid[None, :]
    assert mid.dtype == np.float32 and out.dtype == np.float32
    tiny = np.finfo(np.float32).tiny
    for v in (mid, out):
        assert not ((v != 0) & (np.abs(v) < tiny)).any(), (in_hw, out_hw, filter, at)
    return out


def tile_rows(in_h, out_h, filter, tile=16):
    """Per `tile` output rows, the source rows [ylo, yhi) their taps span, from the bounds table."""
    bounds, _ = detail.aa_coeffs(in_h, out_h, filter)
    return [(int(bounds[y:y + tile, 0].min()), int(bounds[y:y + tile].sum(1).max())) for y in range(0, out_h, tile)]


def impulse_sites(in_hw, out_hw, filter, chunk=32):
    """Where the single non-zero element goes, as (sy, sx) in the window: its four corners and centre, and in the centre
    column the last row of the first LDS chunk and the first row of the second (ylo + chunk - 1, ylo + chunk) of the first
    and of the last output tile, where such a tile spans more than one chunk.  In order, without repeats."""
    h, w = in_hw
    sites = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w // 2)]
    rows = tile_rows(h, out_hw[0], filter)
    for ylo, yhi in (rows[0], rows[-1]):
        if ylo + chunk < yhi:
            sites += [(ylo + chunk - 1, w // 2), (ylo + chunk, w // 2)]
    return list(dict.fromkeys(sites))


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
