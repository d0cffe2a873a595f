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

One region serves every frame of the batch (a video is a batch; the sampler needs one shape); the per-frame form below
moves a window of one size with the mask instead.  HIP tensors only, no CPU fallback; results stay on the device.

Per region, for a mask of several separate areas (two faces at opposite corners share no useful bounding box):

  1. `mask_components`  the mask's 8-connected components on the device (lp_mask_components): a label image that stays there
                        and a table of boxes and areas read back, the job's one device -> host read;
  2. `plan_regions`     host integer arithmetic: components grouped into regions, every region a window of one size;
  3. `crop_regions`     all regions cut out and resampled in one launch (lp_detail_resample_regions), stacked region-major as
                        one sampler batch; region i sees the mask with the components of other regions erased;
  4. `stitch_regions`   the detailed crops back, one frame copy, then region after region in order (lp_detail_stitch_regions):
                        the composition of `stitch` over the regions, bit for bit.

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

The regions rule, in integers.  Components are (r0, r1, c0, c1, area) with labels 1..n in raster order of their first pixel.
  keep     components with area >= min_area.  None left: ValueError ("empty" for an empty mask, naming min_area otherwise).
           Each kept component starts as a group: raw box = its box, members = (its label,).  Groups are always ordered by
           their smallest member label.
  close    a group's window is grow + snap above, on both axes, from its raw box.  While some pair of windows shares a pixel,
           merge the pair lowest in (i, j) order, i < j: union of the raw boxes, union of the members; then start over.
  limit    while there are more than max_regions groups: merge the pair whose union raw box has the smallest area (ties: lowest
           i, then lowest j), then close again.
  equalise h = the largest window height and w = the largest window width over the groups.  Per axis, a window of size n_i at
           lo in an image of size N becomes  lo -= (n - n_i) // 2;  lo = min(max(lo, 0), N - n).  Every region is now h x w
           (equalised windows may overlap; stitch_regions composes them in region order).
  size     (oh, ow) from (h, w, target) by the size rule above: one scale for all regions.
More than LP_DETAIL_MAX_COMPONENTS components (a noise-like mask, the table is truncated): one region from the mask's bounding
box, every label a member.  One group holding every component gives exactly plan_region(mask_bbox(mask), ...).

Per frame, for a mask that moves through a video (a small subject crossing the frame has a union box that is most of the
frame):

  1. `mask_bbox_frames`  one bounding box per frame on the device (lp_mask_bbox_frames, one launch), the [frames, 4] table read
                         back: the job's one device -> host read;
  2. `plan_track`        host integer arithmetic: one window size for the clip and a smoothed path of origins, one per frame;
  3. `crop_track`        every frame's window cut out and resampled in one launch (lp_detail_resample_track);
  4. `stitch_track`      the detailed crops back, one frame copy, then every frame's window in one launch
                         (lp_detail_stitch_track): `stitch` frame by frame, bit for bit.

The track rule, in integers, per axis.  Image size N, frame f's box [a0_f, a1_f] (empty for a frame without a set element),
F frames, c as above, M = multiple_of, k = smooth (odd, >= 1), r = k // 2.  Every division is floor division.
  centre   s_f = a0_f + a1_f + 1, twice the box centre; a window [lo, lo + n) has twice-centre 2 * lo + n.
  fill     an empty frame takes s_f by linear interpolation between the nearest non-empty frames before it (p) and after it
           (q):  s_p + ((s_q - s_p) * (f - p)) // (q - p);  before the first / after the last non-empty frame it holds that
           frame's value.  Every frame empty: ValueError ("the mask is empty ...").
  size     side = the largest a1_f - a0_f + 1 over non-empty frames;  g = padding + ceil((c - 1000) * side / 2000);
           n = min(side + 2 * g, N);  need = ceil(n / M) * M.  If need <= N, n = need; else n stays as grown and is not a
           multiple (as in the region rule).
  smooth   S_f = sum over j = -r..r of s_clamp(f + j, 0, F - 1);  lo_f = (S_f - k * n) // (2 * k).
  contain  non-empty frames only:  lo_f = min(lo_f, a0_f);  lo_f = max(lo_f, a1_f + 1 - n).  n >= side, so both hold: however
           strong the smoothing, a frame's own mask stays inside its window.
  clamp    lo_f = min(max(lo_f, 0), N - n).
  size     (oh, ow) from (h, w, target) by the size rule above: one scale for the whole clip.
A single box with `frames` = B (a static one-plane mask on a batch of B images) stands for B equal boxes and gives B equal
origins.
"""
from __future__ import annotations

import ctypes
import dataclasses
import functools
import math
import typing

import numpy as np
import torch

from . import _cabi
from ._hostcall import int_in, launch, mask3, mask_for, require_hip
from ._util import _as_f32c, tables_for_launch
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
    groups = 1                                            # windows per image

    @property
    def resampled(self):
        return (self.oh, self.ow) != (self.h, self.w)


@dataclasses.dataclass(frozen=True)
class _Windows:
    """Windows [y0, y0 + h) x [x0, x0 + w) of one size in an H x W image, one per `origins` entry, all detailed at (oh, ow)."""
    H: int
    W: int
    h: int
    w: int
    oh: int
    ow: int
    origins: tuple
    groups = 1                                            # windows per image

    def __len__(self):
        return len(self.origins)

    def region(self, i):
        y0, x0 = self.origins[i]
        return Region(y0, x0, self.h, self.w, self.oh, self.ow, self.H, self.W)

    @property
    def resampled(self):
        return (self.oh, self.ow) != (self.h, self.w)


@dataclasses.dataclass(frozen=True)
class Regions(_Windows):
    """One window per region of the mask; `members[i]` are the component labels region i owns, ascending."""
    members: tuple
    groups = property(_Windows.__len__)


@dataclasses.dataclass(frozen=True)
class Track(_Windows):
    """One window per frame of a video: frame f's is at `origins[f]`."""


@dataclasses.dataclass(frozen=True)
class Subjects(_Windows):
    """One window per (subject, frame) (lanpaint_amd/detail_subjects.py): window (s, f) is at `origins[s * frames + f]`;
    `members[s]` are the space-time component labels subject s owns, ascending."""
    frames: int
    members: tuple

    @property
    def subjects(self):
        return len(self.members)

    groups = subjects

    def window(self, s, f):
        return self.region(s * self.frames + f)


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


def _working_size(h, w, m, target):
    if target <= 0:
        return h, w
    long_side = max(h, w)
    return (max(1, (2 * h * target + long_side * m) // (2 * long_side * m)) * m,
            max(1, (2 * w * target + long_side * m) // (2 * long_side * m)) * m)


def _plan_args(H, W, context, padding, multiple_of, target):
    """The planners' shared arguments, checked: (H, W, c1000, padding, m, target) as integers, c1000 = context in thousandths."""
    H, W, padding, m, target = int(H), int(W), int(padding), int(multiple_of), int(target)
    if H <= 0 or W <= 0:
        raise ValueError(f"image size must be positive, got {H}x{W}")
    c1000 = int(round(float(context) * 1000))
    if c1000 < 1000:
        raise ValueError(f"context must be >= 1.0, got {context!r}")
    if padding < 0 or m < 1 or target < 0:
        raise ValueError(f"padding >= 0, multiple_of >= 1 and target >= 0 are required, got {padding}, {m}, {target}")
    return H, W, c1000, padding, m, target


def plan_region(bbox, H, W, context=1.0, padding=0, multiple_of=8, target=0):
    """The module docstring's rule: bbox (r0, r1, c0, c1) inclusive -> Region."""
    r0, r1, c0, c1 = (int(v) for v in bbox)
    H, W, c1000, padding, m, target = _plan_args(H, W, context, padding, multiple_of, target)
    if r1 < r0 or c1 < c0:
        raise ValueError("the mask is empty: there is no region to detail")
    if r0 < 0 or c0 < 0 or r1 >= H or c1 >= W:
        raise ValueError(f"bbox {(r0, r1, c0, c1)} lies outside the {H}x{W} image")
    y0, h = _plan_axis(r0, r1, H, c1000, padding, m)
    x0, w = _plan_axis(c0, c1, W, c1000, padding, m)
    oh, ow = _working_size(h, w, m, target)
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


def _check_filter(filter):
    if filter not in FILTERS:
        raise ValueError(f"filter must be one of {FILTERS}, got {filter!r}")


def _check_region(region, H, W):
    if (region.H, region.W) != (H, W):
        raise ValueError(f"the region was planned for a {region.H}x{region.W} image, got {H}x{W}")


def mask_bbox(mask):
    """(row_min, row_max, col_min, col_max), inclusive, of `mask > 0.5` over every frame of a HIP mask [B, H, W], [1, H, W] or
    [H, W]; (H, -1, W, -1) when nothing is set (plan_region raises on it).  Reads four integers back from the device."""
    m = _as_f32c(mask3(require_hip(mask, "mask", __name__)))
    planes, h, w = m.shape
    dev = m.device
    box = torch.empty(4, dtype=torch.int32, device=dev)
    launch("lp_mask_bbox", dev, m.data_ptr(), planes, h, w, box.data_ptr())
    return tuple(box.cpu().tolist())


def _aa_tables_f32(in_size, out_size, filter):
    """aa_coeffs as the kernel reads it: (bounds int32 [out, 2], weights rounded to float32 [out, ksize])."""
    bounds, weights = aa_coeffs(in_size, out_size, filter)
    return bounds, weights.astype(np.float32)


def _resample(src, win, filter, origins=None, labels=None, owner=None):
    """Every window of `win` cut out of a contiguous fp32 HIP tensor [B, H, W, C] at win's working size through its form's
    crop entry (_FORMS) -> [win.groups * B, oh, ow, C], group-major.  `origins`: the device table of the three table forms;
    `labels` and `owner` (Regions, Subjects): each window is its group's view of a mask."""
    b, sh, sw, c = src.shape
    dev, images, scratch = src.device, win.groups * b, None
    entry = _FORMS[type(win)].crop
    d = _FORMS[type(win)].desc(win, b, sh, sw, c)
    if origins is not None:
        d.origins = origins.data_ptr()
    if labels is not None:
        d.labels, d.owner, d.owner_len = labels.data_ptr(), owner.data_ptr(), owner.numel()
        if win.resampled:
            scratch = torch.empty((images, win.h, win.w), dtype=torch.float32, device=dev)
            d.scratch = scratch.data_ptr()
    out = torch.empty((images, win.oh, win.ow, c), dtype=torch.float32, device=dev)
    d.src, d.dst = src.data_ptr(), out.data_ptr()
    if win.resampled:
        bx, wx = tables_for_launch(_aa_tables_f32, dev, win.w, win.ow, filter)
        by, wy = tables_for_launch(_aa_tables_f32, dev, win.h, win.oh, filter)
        d.ksize_x, d.ksize_y = wx.shape[1], wy.shape[1]
        d.bounds_x, d.weights_x, d.bounds_y, d.weights_y = bx.data_ptr(), wx.data_ptr(), by.data_ptr(), wy.data_ptr()
    launch(entry, dev, ctypes.byref(d))
    return out


def crop_resample(image, mask, region, filter="bilinear"):
    """image [B, H, W, C] and mask ([B, H, W], [1, H, W], [H, W] or None) cut to `region` and resampled to its working size:
    (image [B, oh, ow, C], mask [Bm, oh, ow] or None).  The image takes `filter`, the mask bilinear, and it stays soft."""
    _check_filter(filter)
    img = _as_f32c(require_hip(image, "image", __name__))
    if img.ndim != 4:
        raise ValueError(f"image must be [B, H, W, C], got {tuple(image.shape)}")
    _check_region(region, img.shape[1], img.shape[2])
    r = region
    out = _resample(img, r, filter)
    if mask is None:
        return out, None
    m = _as_f32c(mask3(require_hip(mask, "mask", __name__)))
    if tuple(m.shape[1:]) != (r.H, r.W):
        raise ValueError(f"mask shape {tuple(mask.shape)} does not match images {tuple(image.shape)}")
    return out, _resample(m.unsqueeze(-1), r, "bilinear").squeeze(-1)


def _stitch_inputs(original, detail_img, mask, win, blend_overlap, filter, labels=None, frame_mask=None):
    """What every stitch starts with: the arguments checked against `win` (any of the four forms) and made contiguous fp32 on
    original's device, the crops resampled back to the windows' size in one launch -> (orig, det, m, b, H, W, c).  The mask is
    [B, H, W] or one plane for all images, unless the form has a rule of its own: `frame_mask(mask, B, H, W)`."""
    _check_filter(filter)
    if int_in(blend_overlap, 1, 51, "blend_overlap") % 2 == 0:
        raise ValueError(f"blend_overlap must be an odd integer in 1..51, got {blend_overlap!r}")
    name = _FORMS[type(win)].crops
    orig = _as_f32c(require_hip(original, "original", __name__))
    det = _as_f32c(require_hip(detail_img, name, __name__).to(orig.device))
    if not frame_mask:
        require_hip(mask, "mask", __name__)
    if orig.ndim != 4 or det.ndim != 4:
        raise ValueError(f"original and {name} must be [B, H, W, C]")
    b, H, W, c = orig.shape
    _FORMS[type(win)].check(win, labels, b, H, W)
    want = (win.groups * b, win.oh, win.ow, c)
    if tuple(det.shape) != want:
        raise ValueError(f"{name} must be {want}, got {tuple(det.shape)}")
    m = _as_f32c(frame_mask(mask, b, H, W).to(orig.device)) if frame_mask else mask_for(mask, b, H, W, orig.device)
    if win.resampled:
        det = _resample(det, Region(0, 0, win.oh, win.ow, win.h, win.w, win.oh, win.ow), filter)
    return orig, det, m, b, H, W, c


def stitch(original, detail_img, mask, region, blend_overlap=1, filter="bilinear"):
    """The detailed crop `detail_img` [B, oh, ow, C] back into `original` [B, H, W, C]: resampled to the region's size, blended
    inside the region through MaskBlend's smoothed mask of the whole image (width `blend_overlap`, odd, 1..51), and the
    original bit for bit outside it.  `mask` as for crop_resample: the full-size mask the region was planned from."""
    orig, det, m, b, H, W, c = _stitch_inputs(original, detail_img, mask, region, blend_overlap, filter)
    r, dev = region, orig.device
    out = torch.empty_like(orig)
    d = _cabi.LpDetailStitchDesc(b, H, W, c, r.y0, r.x0, r.h, r.w, blend_overlap, m.shape[0],
                                 m.data_ptr(), orig.data_ptr(), det.data_ptr(), out.data_ptr())
    launch("lp_detail_stitch", dev, ctypes.byref(d))
    return out


# ---- per region --------------------------------------------------------------------------------------------------------------
def mask_components(mask):
    """8-connected components of `mask > 0.5` over every frame of a HIP mask [B, H, W], [1, H, W] or [H, W]:
    (labels int32 [H, W] on the device, n, table).  Labels run 1..n in raster order of each component's first pixel, 0 is the
    background (scipy.ndimage.label with a 3 x 3 structure of ones); table[id - 1] = (r0, r1, c0, c1, area), boxes inclusive,
    for id = 1..min(n, LP_DETAIL_MAX_COMPONENTS).  Reads the table back from the device, nothing else."""
    return _components(mask, "lp_mask_components", 5)


def _components(mask, entry, cols, volume=False):
    """A labelling entry called and its table read back: (labels, n, rows of `cols` integers).  The labels are one image for
    every plane of the mask, or with `volume` one plane each."""
    m = _as_f32c(mask3(require_hip(mask, "mask", __name__)))
    planes, h, w = m.shape
    dev = m.device
    labels = torch.empty((planes, h, w) if volume else (h, w), dtype=torch.int32, device=dev)
    table = torch.empty(1 + cols * _cabi.LP_DETAIL_MAX_COMPONENTS, dtype=torch.int32, device=dev)
    ws_bytes = _cabi.lp_components_frames_ws_bytes(planes, h, w) if volume else _cabi.lp_components_ws_bytes(h, w)
    ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=dev)
    launch(entry, dev, m.data_ptr(), planes, h, w, labels.data_ptr(), table.data_ptr(), ws.data_ptr(), ws_bytes)
    host = table.cpu().numpy()
    n = int(host[0])
    rows = host[1:1 + cols * min(n, _cabi.LP_DETAIL_MAX_COMPONENTS)].reshape(-1, cols)
    return labels, n, tuple(tuple(int(v) for v in row) for row in rows)


def _close(boxes, members, plan):
    """The rule's `close`, in place on the parallel lists `boxes` / `members`.  `cur` walks the groups in order with every pair
    (a, b), a < cur, known to be apart; a merge into `cur` changes only cur's window, so the lowest pair that may newly share a
    pixel is (a, cur) with the smallest such a -- the walk goes back to it -- or else (cur, j) again."""
    win = np.array([plan(b) for b in boxes], np.int64).reshape(-1, 4)
    cur = 0
    while cur < len(boxes):
        y0, h, x0, w = win[cur]
        hit = (win[:, 0] < y0 + h) & (y0 < win[:, 0] + win[:, 1]) & (win[:, 2] < x0 + w) & (x0 < win[:, 2] + win[:, 3])
        hit[cur] = False
        below = np.flatnonzero(hit[:cur])
        if below.size:
            i, j = int(below[0]), cur
        else:
            above = np.flatnonzero(hit[cur + 1:])
            if not above.size:
                cur += 1
                continue
            i, j = cur, cur + 1 + int(above[0])
        a, b = boxes[i], boxes[j]
        boxes[i] = (min(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), max(a[3], b[3]))
        members[i] = tuple(sorted(members[i] + members[j]))
        del boxes[j], members[j]
        win = np.delete(win, j, axis=0)
        win[i] = plan(boxes[i])
        cur = i


def _merge_smallest_union(boxes, members):
    """A rule's `limit`, one merge: the pair (i, j), i < j, whose union box -- (lo, hi) inclusive per axis, any number of axes --
    has the smallest product of extents; ties to the lowest i, then j."""
    b = np.array(boxes, np.int64)
    size = np.ones((len(boxes), len(boxes)), np.int64)
    for a in range(0, b.shape[1], 2):
        size *= np.maximum(b[:, None, a + 1], b[None, :, a + 1]) - np.minimum(b[:, None, a], b[None, :, a]) + 1
    size[np.tril_indices(len(boxes))] = np.iinfo(np.int64).max
    i, j = (int(v) for v in np.unravel_index(int(np.argmin(size)), size.shape))      # argmin: the first in row-major order
    p, q = boxes[i], boxes[j]
    boxes[i] = tuple(min(p[a], q[a]) if a % 2 == 0 else max(p[a], q[a]) for a in range(len(p)))
    members[i] = tuple(sorted(members[i] + members[j]))
    del boxes[j], members[j]


def plan_regions(components, H, W, context=1.0, padding=0, multiple_of=8, target=0, min_area=1, max_regions=8, bbox=None):
    """The module docstring's regions rule.  `components` = (n, table) as mask_components returns them after the label image
    (the 3-tuple itself is taken too) -> Regions.  `bbox`, the mask's bounding box (mask_bbox), is needed only when
    n > LP_DETAIL_MAX_COMPONENTS, where the table is truncated and one region serves the whole mask."""
    n, table = components[-2], components[-1]
    H, W, c1000, padding, m, target = _plan_args(H, W, context, padding, multiple_of, target)
    n, min_area, max_regions = int(n), int(min_area), int(max_regions)
    if min_area < 1 or max_regions < 1:
        raise ValueError(f"min_area >= 1 and max_regions >= 1 are required, got {min_area}, {max_regions}")
    if n <= 0:
        raise ValueError("the mask is empty: there is no region to detail")
    if n > _cabi.LP_DETAIL_MAX_COMPONENTS:
        if bbox is None:
            raise ValueError(f"{n} components exceed the table's {_cabi.LP_DETAIL_MAX_COMPONENTS}: pass bbox=mask_bbox(mask) "
                             "to plan the single region that serves such a mask")
        r = plan_region(bbox, H, W, context, padding, m, target)
        return Regions(H, W, r.h, r.w, r.oh, r.ow, ((r.y0, r.x0),), (tuple(range(1, n + 1)),))
    if len(table) != n:
        raise ValueError(f"the table holds {len(table)} components, the count says {n}")
    boxes, members = [], []
    for label, (r0, r1, c0, c1, area) in enumerate(table, 1):
        if r0 < 0 or c0 < 0 or r1 >= H or c1 >= W or r1 < r0 or c1 < c0:
            raise ValueError(f"component {label}'s box {(r0, r1, c0, c1)} lies outside the {H}x{W} image")
        if area >= min_area:
            boxes.append((int(r0), int(r1), int(c0), int(c1)))
            members.append((label,))
    if not boxes:
        raise ValueError(f"min_area = {min_area} leaves none of the mask's {n} components: there is no region to detail")

    def plan(box):
        return _plan_axis(box[0], box[1], H, c1000, padding, m) + _plan_axis(box[2], box[3], W, c1000, padding, m)

    _close(boxes, members, plan)
    while len(boxes) > max_regions:
        _merge_smallest_union(boxes, members)
        _close(boxes, members, plan)
    win = [plan(b) for b in boxes]
    h, w = max(v[1] for v in win), max(v[3] for v in win)
    origins = tuple((min(max(y0 - (h - hi) // 2, 0), H - h), min(max(x0 - (w - wi) // 2, 0), W - w)) for y0, hi, x0, wi in win)
    oh, ow = _working_size(h, w, m, target)
    return Regions(H, W, h, w, oh, ow, origins, tuple(members))


def _origins_table(win, dev):
    """win's origins as the table forms' entries read them: int32 [n, 2] on the device."""
    return torch.tensor(win.origins, dtype=torch.int32, device=dev).reshape(-1, 2)


def _owner_table(members, dev):
    """owner int32 on the device: owner[label] = group + 1, 0 for a label no region or subject owns."""
    owner = np.zeros(max(max(mem) for mem in members) + 1, np.int32)
    for i, mem in enumerate(members):
        owner[np.asarray(mem, np.int64)] = i + 1
    return torch.from_numpy(owner).to(dev)


def _check_labels(labels, planes, H, W):
    """`planes`: None for one label image (mask_components), else the planes of a label volume (mask_components_frames)."""
    require_hip(labels, "labels", __name__)
    shape, source = ((H, W), "mask_components") if planes is None else ((planes, H, W), "mask_components_frames")
    if labels.dtype != torch.int32 or tuple(labels.shape) != shape or not labels.is_contiguous():
        raise ValueError(f"labels must be a contiguous int32 {list(shape)} tensor ({source}), got {labels.dtype} "
                         f"{tuple(labels.shape)}")


def _check_regions(regions, labels, H, W):
    if (regions.H, regions.W) != (H, W):
        raise ValueError(f"the regions were planned for a {regions.H}x{regions.W} image, got {H}x{W}")
    if not 1 <= len(regions) <= _cabi.LP_DETAIL_MAX_REGIONS:
        raise ValueError(f"1..{_cabi.LP_DETAIL_MAX_REGIONS} regions are supported, got {len(regions)}")
    if labels is not None:
        _check_labels(labels, None, H, W)


def crop_regions(image, mask, regions, labels=None, filter="bilinear"):
    """crop_resample for every region at once: (image [R * B, oh, ow, C], mask [R * Bm, oh, ow] or None), region-major, so the
    stack is one sampler batch.  Region i's mask is `mask` with the components of other regions -- and those min_area dropped
    -- set to 0 (`labels` from mask_components; None: the mask as it is); values at or below 0.5 are nobody's and stay."""
    _check_filter(filter)
    img = _as_f32c(require_hip(image, "image", __name__))
    if img.ndim != 4:
        raise ValueError(f"image must be [B, H, W, C], got {tuple(image.shape)}")
    H, W = img.shape[1], img.shape[2]
    _check_regions(regions, labels, H, W)
    origins = _origins_table(regions, img.device)
    owner = None if labels is None else _owner_table(regions.members, img.device)
    out = _resample(img, regions, filter, origins)
    if mask is None:
        return out, None
    m = _as_f32c(mask3(require_hip(mask, "mask", __name__)).to(img.device))
    if tuple(m.shape[1:]) != (H, W):
        raise ValueError(f"mask shape {tuple(mask.shape)} does not match images {tuple(image.shape)}")
    return out, _resample(m.unsqueeze(-1), regions, "bilinear", origins, labels, owner).squeeze(-1)


def stitch_regions(original, detail_imgs, mask, regions, labels=None, blend_overlap=1, filter="bilinear"):
    """The detailed crops `detail_imgs` [R * B, oh, ow, C] (region-major, as crop_regions stacks them) back into `original`
    [B, H, W, C].  The result is the composition of `stitch` in region order,  out_0 = original,  out_{i+1} = stitch(out_i,
    detail_i, mask_i, region i),  bit for bit -- equalised windows may overlap, so the order counts -- computed as one copy of
    the frame and then each region's window in place."""
    orig, det, m, b, H, W, c = _stitch_inputs(original, detail_imgs, mask, regions, blend_overlap, filter, labels)
    g, n_reg, k, dev = regions, len(regions), blend_overlap, orig.device
    host_origins = (ctypes.c_int32 * (2 * n_reg))(*(v for o in g.origins for v in o))
    out = torch.empty_like(orig)
    d = _cabi.LpDetailStitchRegionsDesc(b, H, W, c, n_reg, g.h, g.w, k, m.shape[0], 0)
    d.origins = ctypes.cast(host_origins, ctypes.c_void_p)
    d.mask, d.original, d.detail, d.out = m.data_ptr(), orig.data_ptr(), det.data_ptr(), out.data_ptr()
    if labels is not None:
        owner = _owner_table(g.members, dev)
        d.labels, d.owner, d.owner_len = labels.data_ptr(), owner.data_ptr(), owner.numel()
    launch("lp_detail_stitch_regions", dev, ctypes.byref(d))
    return out


# ---- per frame: a window that follows a moving mask --------------------------------------------------------------------------------
def _track_size(side, n_img, c1000, padding, m):
    """The track rule's first `size` step on one axis: the window size for boxes whose largest side is `side`."""
    g = padding + _ceil_div((c1000 - 1000) * side, 2000)
    n = min(side + 2 * g, n_img)
    need = _ceil_div(n, m) * m
    return need if need <= n_img else n


def _track_axis(spans, n_img, c1000, padding, m, k, n=None):
    """One axis of the track rule: spans[f] = (a0, a1) inclusive, or None for an empty frame -> (origins, n).  `n`: the window
    size when the caller has fixed it (at least the largest side), otherwise the rule's own from these spans."""
    frames = len(spans)
    full = [f for f, span in enumerate(spans) if span is not None]
    s = [None if span is None else span[0] + span[1] + 1 for span in spans]
    for f in range(frames):                                               # fill
        if s[f] is None:
            before = [p for p in full if p < f]
            after = [q for q in full if q > f]
            if before and after:
                p, q = before[-1], after[0]
                s[f] = s[p] + ((s[q] - s[p]) * (f - p)) // (q - p)
            else:
                s[f] = s[before[-1] if before else after[0]]
    if n is None:                                                         # size
        n = _track_size(max(spans[f][1] - spans[f][0] + 1 for f in full), n_img, c1000, padding, m)
    origins = []
    for f in range(frames):
        total = sum(s[min(max(f + j, 0), frames - 1)] for j in range(-(k // 2), k // 2 + 1))     # smooth
        lo = (total - k * n) // (2 * k)
        if spans[f] is not None:                                          # contain
            lo = max(min(lo, spans[f][0]), spans[f][1] + 1 - n)
        origins.append(min(max(lo, 0), n_img - n))                        # clamp
    return origins, n


def _check_smooth(smooth):
    if isinstance(smooth, bool) or int(smooth) != smooth or smooth < 1 or smooth % 2 == 0:
        raise ValueError(f"smooth must be an odd integer >= 1, got {smooth!r}")
    return int(smooth)


def _box_spans(boxes, H, W, what):
    """One path's boxes (r0, r1, c0, c1), inclusive, as the row spans and the column spans _track_axis takes: None for an empty
    frame (r1 < r0).  `what(f)` names frame f's box in the error for one outside the image."""
    rows, cols = [], []
    for f, (r0, r1, c0, c1) in enumerate(boxes):
        if r1 < r0 or c1 < c0:
            rows.append(None)
            cols.append(None)
            continue
        if r0 < 0 or c0 < 0 or r1 >= H or c1 >= W:
            raise ValueError(f"{what(f)} {(r0, r1, c0, c1)} lies outside the {H}x{W} image")
        rows.append((r0, r1))
        cols.append((c0, c1))
    return rows, cols


def plan_track(boxes, H, W, context=1.0, padding=0, multiple_of=8, target=0, smooth=1, frames=None):
    """The module docstring's track rule: one box (r0, r1, c0, c1) per frame, inclusive, empty frames as lp_mask_bbox marks
    them (r1 < r0) -> Track.  `frames` is the length of the batch the track serves: len(boxes) when not given, and a single
    box is repeated to it (a static mask)."""
    boxes = [tuple(int(v) for v in box) for box in boxes]
    H, W, c1000, padding, m, target = _plan_args(H, W, context, padding, multiple_of, target)
    smooth = _check_smooth(smooth)
    frames = len(boxes) if frames is None else int(frames)
    if frames < 1 or len(boxes) not in (1, frames) or any(len(box) != 4 for box in boxes):
        raise ValueError(f"one box of four integers per frame, or a single one, is required: got {len(boxes)} for {frames} frames")
    if len(boxes) != frames:
        boxes = boxes * frames
    rows, cols = _box_spans(boxes, H, W, lambda f: f"frame {f}'s box")
    if all(span is None for span in rows):
        raise ValueError("the mask is empty in every frame: there is no region to detail")
    ys, h = _track_axis(rows, H, c1000, padding, m, smooth)
    xs, w = _track_axis(cols, W, c1000, padding, m, smooth)
    oh, ow = _working_size(h, w, m, target)
    return Track(H, W, h, w, oh, ow, tuple(zip(ys, xs)))


def mask_bbox_frames(mask):
    """`mask_bbox` of every frame on its own, in one launch: a tuple of (row_min, row_max, col_min, col_max), one per plane of a
    HIP mask [B, H, W], [1, H, W] or [H, W]; (H, -1, W, -1) for a frame with nothing set.  Reads the [B, 4] table back."""
    m = _as_f32c(mask3(require_hip(mask, "mask", __name__)))
    planes, h, w = m.shape
    dev = m.device
    boxes = torch.empty((planes, 4), dtype=torch.int32, device=dev)
    launch("lp_mask_bbox_frames", dev, m.data_ptr(), planes, h, w, boxes.data_ptr())
    return tuple(tuple(row) for row in boxes.cpu().tolist())


def _check_track(track, batch, H, W):
    if (track.H, track.W) != (H, W):
        raise ValueError(f"the track was planned for a {track.H}x{track.W} image, got {H}x{W}")
    if len(track) != batch:
        raise ValueError(f"the track holds {len(track)} frames, the batch {batch}")
    _check_fit(track, H, W, lambda f: f"frame {f}'s window")


def _check_fit(win, H, W, what):
    """Every window of a table form lies inside the H x W image; `what(i)` names window i in the error."""
    if not (0 < win.h <= H and 0 < win.w <= W):
        raise ValueError(f"a {win.h}x{win.w} window does not fit the {H}x{W} image")
    for i, (y0, x0) in enumerate(win.origins):
        if y0 < 0 or x0 < 0 or y0 + win.h > H or x0 + win.w > W:
            raise ValueError(f"{what(i)} at {(y0, x0)} leaves the {H}x{W} image")


def _check_members(members):
    members = tuple(tuple(int(v) for v in mem) for mem in members)
    if not 1 <= len(members) <= _cabi.LP_DETAIL_MAX_REGIONS:
        raise ValueError(f"1..{_cabi.LP_DETAIL_MAX_REGIONS} subjects are supported, got {len(members)}")
    if any(not mem or min(mem) < 1 for mem in members):
        raise ValueError("every subject needs at least one member label, and labels start at 1")
    return members


def _check_subjects(subjects, labels, frames, H, W):
    if (subjects.H, subjects.W) != (H, W):
        raise ValueError(f"the subjects were planned for a {subjects.H}x{subjects.W} image, got {H}x{W}")
    if subjects.frames != frames or len(subjects.origins) != subjects.subjects * frames:
        raise ValueError(f"the subjects were planned for {subjects.frames} frames, the batch holds {frames}")
    _check_members(subjects.members)
    _check_fit(subjects, H, W, lambda i: f"subject {i // frames}, frame {i % frames}: the window")
    if labels is not None:
        _check_labels(labels, frames, H, W)


class _Form(typing.NamedTuple):
    """What differs between the four forms behind _resample and _stitch_inputs, by window class."""
    crop: str                                             # the crop entry
    desc: typing.Callable                                 # (win, b, sh, sw, c) -> its descriptor, up to the pointers
    check: typing.Callable                                # (win, labels, b, H, W): the windows against a batch, or ValueError
    crops: str                                            # what the stitch calls its crops


_FORMS = {
    Region: _Form("lp_detail_resample",
                  lambda r, *src: _cabi.LpDetailResampleDesc(*src, r.y0, r.x0, r.h, r.w, r.oh, r.ow),
                  lambda r, labels, b, H, W: _check_region(r, H, W), "detail_img"),
    Regions: _Form("lp_detail_resample_regions",
                   lambda g, *src: _cabi.LpDetailResampleRegionsDesc(*src, g.groups, g.h, g.w, 0, g.oh, g.ow),
                   lambda g, labels, b, H, W: _check_regions(g, labels, H, W), "detail_imgs"),
    Track: _Form("lp_detail_resample_track",
                 lambda t, *src: _cabi.LpDetailResampleTrackDesc(*src, t.h, t.w, t.oh, t.ow),
                 lambda t, labels, b, H, W: _check_track(t, b, H, W), "detail_img"),
    Subjects: _Form("lp_detail_resample_subjects",
                    lambda g, *src: _cabi.LpDetailResampleSubjectsDesc(*src, g.groups, g.h, g.w, 0, g.oh, g.ow),
                    _check_subjects, "detail_imgs"),
}


def crop_track(image, mask, track, filter="bilinear"):
    """crop_resample with frame f cut at `track.region(f)`: (image [B, oh, ow, C], mask [Bm, oh, ow] or None), each frame what
    crop_resample gives for it alone, bit for bit.  A one-plane mask stays one plane while the track stands still (plan_track
    of a static mask); under a track that moves it is cut once per frame, [B, oh, ow]."""
    _check_filter(filter)
    img = _as_f32c(require_hip(image, "image", __name__))
    if img.ndim != 4:
        raise ValueError(f"image must be [B, H, W, C], got {tuple(image.shape)}")
    b, H, W = img.shape[0], img.shape[1], img.shape[2]
    _check_track(track, b, H, W)
    origins = _origins_table(track, img.device)
    out = _resample(img, track, filter, origins)
    if mask is None:
        return out, None
    m = mask_for(require_hip(mask, "mask", __name__), b, H, W, img.device)
    if m.shape[0] != b:
        if len(set(track.origins)) == 1:
            origins = origins[:1]
        else:
            m = m.expand(b, H, W)
    return out, _resample(_as_f32c(m).unsqueeze(-1), track, "bilinear", origins).squeeze(-1)


def stitch_track(original, detail_img, mask, track, blend_overlap=1, filter="bilinear"):
    """`stitch` with frame f's crop put back at `track.region(f)`: the detailed crops `detail_img` [B, oh, ow, C] into
    `original` [B, H, W, C], frame by frame what `stitch` gives, bit for bit, as one copy of the frames and one launch over
    every frame's window.  `mask` [B, H, W] or one plane for all frames."""
    orig, det, m, b, H, W, c = _stitch_inputs(original, detail_img, mask, track, blend_overlap, filter)
    t, k, dev = track, blend_overlap, orig.device
    origins = _origins_table(t, dev)
    out = torch.empty_like(orig)
    d = _cabi.LpDetailStitchTrackDesc(b, H, W, c, t.h, t.w, k, m.shape[0],
                                      origins.data_ptr(), m.data_ptr(), orig.data_ptr(), det.data_ptr(), out.data_ptr())
    launch("lp_detail_stitch_track", dev, ctypes.byref(d))
    return out
