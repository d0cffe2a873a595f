"""Detailer per subject of a video: several masked subjects that move, each followed by a window of its own.

The three forms of lanpaint_amd/detail.py each miss this case: the single crop has one box for the whole mask; the regions
form labels the union of the mask over frames, where one walking person is a smear as wide as their path and two people whose
paths cross are one component; the track form has one box per frame, which spans every subject in it.  Here the mask is
labelled in space and time, so that "the same blob one frame later" is the same component, and the regions' erasure and the
track's window policy are combined per (subject, frame):

  1. `mask_components_frames`  the mask's 26-connected components in (f, y, x) on the device (lp_mask_components_frames): a
                               label volume that stays there and a table of space-time boxes and volumes read back, the job's
                               first device -> host read (n and 7 integers per component, about 112 KB at the cap);
  2. `group_subjects`          host integer arithmetic: components grouped into subjects;
  3. `subject_boxes`           one bounding box per (subject, frame) on the device (lp_subject_boxes, one launch), the
                               [subjects, frames, 4] table read back: the job's second and last device -> host read (about
                               83 KB at 64 subjects x 81 frames);
  4. `plan_subjects`           host integer arithmetic: one window size for the job and a smoothed path of origins per subject;
  5. `crop_subjects`           every (subject, frame) window cut out and resampled in one launch
                               (lp_detail_resample_subjects), stacked subject-major as one sampler batch; subject s sees frame
                               f's mask with the components of other subjects erased;
  6. `stitch_subjects`         the detailed crops back, one frame copy, then subject after subject in order, each over all
                               frames' windows in one launch (lp_detail_stitch_subjects): the composition of `stitch` over
                               subjects and frames, bit for bit.

The subjects rule, in integers.  Components are (f0, f1, r0, r1, c0, c1, volume), bounds inclusive, with labels 1..n in raster
order of their first voxel.  F frames, image H x W; c, M, k as in detail.py's rules.
  keep     components with volume >= min_area * (f1 - f0 + 1): a mean area over their life of at least min_area.  None left:
           ValueError ("empty" for an empty mask, naming min_area otherwise, in the regions rule's words).  Each kept
           component starts as a subject with members = (its label,).  Subjects are always ordered by their smallest member
           label.
  no close unlike the regions rule there is no `close` step: two subjects whose windows overlap but whose masks do not touch
           stay apart.  The stitch composes them in subject order, and each changes only pixels under its own mask's smoothed
           support, so overlapping windows do no harm -- and merging them is what this form exists to avoid.
  limit    while there are more than max_subjects: merge the pair (i < j) whose union space-time box has the smallest product
           frame extent * row extent * col extent (ties: lowest i, then lowest j); the merged subject holds the union of the
           members, sorted.
  past the cap  n > LP_DETAIL_MAX_COMPONENTS (a noise-like mask, the table is truncated): one subject that owns every label.  Its
           boxes are mask_bbox_frames' (subject_boxes gives the same: a label is non-zero exactly where the mask is set), and
           the plan is exactly plan_track's.
  size     per axis, side = the largest box side over all subjects and all their non-empty frames; g, n and need follow as in
           the track rule's `size` step.  One window size (h, w) and one working size (oh, ow) for the whole job.
  path     per subject and axis, the track rule's fill, smooth, contain and clamp with that n.  Frames where the subject is
           absent are bridged or held like an empty frame in plan_track.
  result   Subjects: window (s, f) is at origins[s * F + f], subject-major.
A single subject that is the only component gives plan_track(mask_bbox_frames(mask), ...) exactly.

HIP tensors only, no CPU fallback; results stay on the device.  The mask has one plane per image.
"""
from __future__ import annotations

import ctypes
import dataclasses

import numpy as np
import torch

from . import _cabi, detail
from ._util import _as_f32c, device_tables, raw_stream
from .detail import Region, _Windows, _check_filter, _mask3


@dataclasses.dataclass(frozen=True)
class Subjects(_Windows):
    """One window per (subject, frame): window (s, f) is at `origins[s * frames + f]`; `members[s]` are the space-time component
    labels subject s owns, ascending."""
    frames: int
    members: tuple

    @property
    def subjects(self):
        return len(self.members)

    def window(self, s, f):
        return self.region(s * self.frames + f)


def _hip(t, what):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"lanpaint_amd.detail_subjects runs on a HIP device only; no CPU fallback ({what} is not on one)")
    return t


def _frame_mask(mask, frames, H, W):
    """The mask as [frames, H, W]: one plane per image."""
    m = _mask3(mask if torch.is_tensor(mask) else _hip(mask, "mask"))
    if m.shape[0] == 1 and frames > 1:
        raise ValueError(f"the subjects form needs one mask plane per image, got one plane for {frames} images: a mask that "
                         "stands still is served by the region nodes (LanPaint_DetailerCropRegions)")
    if m.shape[0] != frames or tuple(m.shape[1:]) != (H, W):
        raise ValueError(f"mask shape {tuple(mask.shape)} does not match {frames} images of {H}x{W}")
    return _hip(m, "mask")


def mask_components_frames(mask):
    """26-connected components of `mask > 0.5` in (f, y, x) of a HIP mask [F, H, W] (or [H, W], one frame), no union over
    planes: (labels int32 [F, H, W] on the device, n, table).  Labels run 1..n in raster order of each component's first voxel,
    0 is the background (scipy.ndimage.label with a 3 x 3 x 3 structure of ones); table[id - 1] = (f0, f1, r0, r1, c0, c1,
    volume), bounds inclusive, for id = 1..min(n, LP_DETAIL_MAX_COMPONENTS).  Reads the table back from the device: the first of
    a job's two reads."""
    m = _as_f32c(_mask3(_hip(mask, "mask")))
    frames, h, w = m.shape
    dev = m.device
    labels = torch.empty((frames, h, w), dtype=torch.int32, device=dev)
    table = torch.empty(1 + 7 * _cabi.LP_DETAIL_MAX_COMPONENTS, dtype=torch.int32, device=dev)
    ws_bytes = _cabi.lp_components_frames_ws_bytes(frames, h, w)
    ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _cabi.check(_cabi.load().lp_mask_components_frames(m.data_ptr(), frames, h, w, labels.data_ptr(), table.data_ptr(),
                                                           ws.data_ptr(), ws_bytes, raw_stream(dev)),
                    "lp_mask_components_frames")
    host = table.cpu().numpy()
    n = int(host[0])
    rows = host[1:1 + 7 * min(n, _cabi.LP_DETAIL_MAX_COMPONENTS)].reshape(-1, 7)
    return labels, n, tuple(tuple(int(v) for v in row) for row in rows)


def _merge_smallest_volume(boxes, members):
    """The rule's `limit`, one merge: the pair (i, j), i < j, whose union space-time box is smallest; ties to the lowest i, then j."""
    b = np.array(boxes, np.int64)
    vol = np.ones((len(boxes), len(boxes)), np.int64)
    for a in (0, 2, 4):
        vol *= np.maximum(b[:, None, a + 1], b[None, :, a + 1]) - np.minimum(b[:, None, a], b[None, :, a]) + 1
    vol[np.tril_indices(len(boxes))] = np.iinfo(np.int64).max
    i, j = (int(v) for v in np.unravel_index(int(np.argmin(vol)), vol.shape))        # argmin: the first in row-major order
    p, q = boxes[i], boxes[j]
    boxes[i] = tuple(min(p[a], q[a]) if a % 2 == 0 else max(p[a], q[a]) for a in range(6))
    members[i] = tuple(sorted(members[i] + members[j]))
    del boxes[j], members[j]


def group_subjects(components, min_area=1, max_subjects=4):
    """The module docstring's keep and limit steps.  `components` = (n, table) as mask_components_frames returns them after the
    label volume (the 3-tuple itself is taken too) -> members, a tuple of tuples of labels, one per subject."""
    n, table = int(components[-2]), components[-1]
    min_area, max_subjects = int(min_area), int(max_subjects)
    if min_area < 1 or max_subjects < 1:
        raise ValueError(f"min_area >= 1 and max_subjects >= 1 are required, got {min_area}, {max_subjects}")
    if n <= 0:
        raise ValueError("the mask is empty: there is no region to detail")
    if n > _cabi.LP_DETAIL_MAX_COMPONENTS:
        return (tuple(range(1, n + 1)),)
    if len(table) != n:
        raise ValueError(f"the table holds {len(table)} components, the count says {n}")
    boxes, members = [], []
    for label, row in enumerate(table, 1):
        f0, f1, r0, r1, c0, c1, volume = (int(v) for v in row)
        if f0 < 0 or r0 < 0 or c0 < 0 or f1 < f0 or r1 < r0 or c1 < c0:
            raise ValueError(f"component {label}'s box {(f0, f1, r0, r1, c0, c1)} is not one")
        if volume >= min_area * (f1 - f0 + 1):
            boxes.append((f0, f1, r0, r1, c0, c1))
            members.append((label,))
    if not boxes:
        raise ValueError(f"min_area = {min_area} leaves none of the mask's {n} components: there is no region to detail")
    while len(boxes) > max_subjects:
        _merge_smallest_volume(boxes, members)
    return tuple(members)


def _check_members(members):
    members = tuple(tuple(int(v) for v in mem) for mem in members)
    if not 1 <= len(members) <= _cabi.LP_DETAIL_MAX_REGIONS:
        raise ValueError(f"1..{_cabi.LP_DETAIL_MAX_REGIONS} subjects are supported, got {len(members)}")
    if any(not mem or min(mem) < 1 for mem in members):
        raise ValueError("every subject needs at least one member label, and labels start at 1")
    return members


def _owner_table(members, dev):
    """owner int32 on the device: owner[label] = subject + 1, 0 for a label no subject owns."""
    owner = np.zeros(max(max(mem) for mem in members) + 1, np.int32)
    for i, mem in enumerate(members):
        owner[np.asarray(mem, np.int64)] = i + 1
    return torch.from_numpy(owner).to(dev)


def _check_labels(labels, frames, H, W):
    _hip(labels, "labels")
    if labels.dtype != torch.int32 or tuple(labels.shape) != (frames, H, W) or not labels.is_contiguous():
        raise ValueError(f"labels must be a contiguous int32 [{frames}, {H}, {W}] tensor (mask_components_frames), got "
                         f"{labels.dtype} {tuple(labels.shape)}")


def subject_boxes(labels, members):
    """One bounding box per (subject, frame): boxes[s][f] = (row_min, row_max, col_min, col_max), inclusive, over the voxels of
    frame f whose label is one of members[s]; (H, -1, W, -1) for a frame the subject is absent from.  One launch
    (lp_subject_boxes); reads the [subjects, frames, 4] table back: the second of a job's two reads."""
    _hip(labels, "labels")
    if labels.ndim != 3:
        raise ValueError(f"labels must be [F, H, W], got {tuple(labels.shape)}")
    frames, h, w = labels.shape
    _check_labels(labels, frames, h, w)
    members = _check_members(members)
    dev = labels.device
    owner = _owner_table(members, dev)
    boxes = torch.empty((len(members), frames, 4), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _cabi.check(_cabi.load().lp_subject_boxes(labels.data_ptr(), frames, h, w, owner.data_ptr(), owner.numel(), len(members),
                                                  boxes.data_ptr(), raw_stream(dev)), "lp_subject_boxes")
    return tuple(tuple(tuple(row) for row in sub) for sub in boxes.cpu().tolist())


def plan_subjects(members, boxes, H, W, context=1.0, padding=0, multiple_of=8, target=0, smooth=1):
    """The module docstring's size, path and result steps: `members` from group_subjects, boxes[s][f] = (r0, r1, c0, c1)
    inclusive from subject_boxes, an absent frame as lp_subject_boxes marks it (r1 < r0) -> Subjects."""
    members = _check_members(members)
    H, W, c1000, padding, m, target = detail._plan_args(H, W, context, padding, multiple_of, target)
    if isinstance(smooth, bool) or int(smooth) != smooth or smooth < 1 or smooth % 2 == 0:
        raise ValueError(f"smooth must be an odd integer >= 1, got {smooth!r}")
    boxes = [[tuple(int(v) for v in box) for box in sub] for sub in boxes]
    frames = len(boxes[0]) if boxes else 0
    if len(boxes) != len(members) or frames < 1 or any(len(sub) != frames for sub in boxes) or \
            any(len(box) != 4 for sub in boxes for box in sub):
        raise ValueError(f"one row of boxes per subject and one box of four integers per frame are required: got {len(boxes)} "
                         f"rows for {len(members)} subjects")
    rows, cols = [], []
    for s, sub in enumerate(boxes):
        rs, cs = [], []
        for f, (r0, r1, c0, c1) in enumerate(sub):
            if r1 < r0 or c1 < c0:
                rs.append(None)
                cs.append(None)
                continue
            if r0 < 0 or c0 < 0 or r1 >= H or c1 >= W:
                raise ValueError(f"subject {s}, frame {f}: box {(r0, r1, c0, c1)} lies outside the {H}x{W} image")
            rs.append((r0, r1))
            cs.append((c0, c1))
        if all(span is None for span in rs):
            raise ValueError(f"subject {s} is in no frame: the mask is empty in every frame of it, there is no region to detail")
        rows.append(rs)
        cols.append(cs)
    h = detail._track_size(max(sp[1] - sp[0] + 1 for rs in rows for sp in rs if sp is not None), H, c1000, padding, m)
    w = detail._track_size(max(sp[1] - sp[0] + 1 for cs in cols for sp in cs if sp is not None), W, c1000, padding, m)
    origins = []
    for rs, cs in zip(rows, cols):
        ys, _ = detail._track_axis(rs, H, c1000, padding, m, int(smooth), h)
        xs, _ = detail._track_axis(cs, W, c1000, padding, m, int(smooth), w)
        origins.extend(zip(ys, xs))
    oh, ow = detail._working_size(h, w, m, target)
    return Subjects(H, W, h, w, oh, ow, tuple(origins), frames, members)


def _check_subjects(subjects, labels, frames, H, W):
    if (subjects.H, subjects.W) != (H, W):
        raise ValueError(f"the subjects were planned for a {subjects.H}x{subjects.W} image, got {H}x{W}")
    if subjects.frames != frames or len(subjects.origins) != subjects.subjects * frames:
        raise ValueError(f"the subjects were planned for {subjects.frames} frames, the batch holds {frames}")
    _check_members(subjects.members)
    if not (0 < subjects.h <= H and 0 < subjects.w <= W):
        raise ValueError(f"a {subjects.h}x{subjects.w} window does not fit the {H}x{W} image")
    for i, (y0, x0) in enumerate(subjects.origins):
        if y0 < 0 or x0 < 0 or y0 + subjects.h > H or x0 + subjects.w > W:
            raise ValueError(f"subject {i // frames}, frame {i % frames}: the window at {(y0, x0)} leaves the {H}x{W} image")
    if labels is not None:
        _check_labels(labels, frames, H, W)


def _origins(subjects, dev):
    return torch.tensor(subjects.origins, dtype=torch.int32, device=dev).reshape(-1, 2)


def _resample(src, win, filter, origins, labels=None, owner=None):
    """Every (subject, frame) window of `win` cut out of a contiguous fp32 HIP tensor [F, H, W, C] at win's working size through
    lp_detail_resample_subjects -> [S * F, oh, ow, C]; with `labels` and `owner` subject s's view of a mask."""
    b, sh, sw, c = src.shape
    dev, images, scratch = src.device, win.subjects * b, None
    d = _cabi.LpDetailResampleSubjectsDesc(b, sh, sw, c, win.subjects, win.h, win.w, 0, win.oh, win.ow,
                                           origins=origins.data_ptr())
    if labels is not None:
        d.labels, d.owner, d.owner_len = labels.data_ptr(), owner.data_ptr(), owner.numel()
        if win.resampled:
            scratch = torch.empty((images, win.h, win.w), dtype=torch.float32, device=dev)
            d.scratch = scratch.data_ptr()
    out = torch.empty((images, win.oh, win.ow, c), dtype=torch.float32, device=dev)
    d.src, d.dst = src.data_ptr(), out.data_ptr()
    if win.resampled:
        bx, wx = device_tables(detail._aa_tables_f32, dev, win.w, win.ow, filter)
        by, wy = device_tables(detail._aa_tables_f32, dev, win.h, win.oh, filter)
        d.ksize_x, d.ksize_y = wx.shape[1], wy.shape[1]
        d.bounds_x, d.weights_x, d.bounds_y, d.weights_y = bx.data_ptr(), wx.data_ptr(), by.data_ptr(), wy.data_ptr()
    with torch.cuda.device(dev):
        _cabi.check(_cabi.load().lp_detail_resample_subjects(ctypes.byref(d), raw_stream(dev)), "lp_detail_resample_subjects")
    return out


def crop_subjects(image, mask, subjects, labels=None, filter="bilinear"):
    """crop_resample for every (subject, frame) at once: (image [S * F, oh, ow, C], mask [S * F, oh, ow] or None),
    subject-major, so the stack is one sampler batch: entry s * F + f is frame f cut at `subjects.window(s, f)`.  Subject s's
    mask is frame f's with the components of other subjects -- and those min_area dropped -- set to 0 (`labels` from
    mask_components_frames; None: the mask as it is); values at or below 0.5 are nobody's and stay."""
    _check_filter(filter)
    img = _as_f32c(_hip(image, "image"))
    if img.ndim != 4:
        raise ValueError(f"image must be [B, H, W, C], got {tuple(image.shape)}")
    frames, H, W = img.shape[0], img.shape[1], img.shape[2]
    _check_subjects(subjects, labels, frames, H, W)
    origins = _origins(subjects, img.device)
    out = _resample(img, subjects, filter, origins)
    if mask is None:
        return out, None
    m = _as_f32c(_frame_mask(mask, frames, H, W).to(img.device))
    owner = None if labels is None else _owner_table(subjects.members, img.device)
    return out, _resample(m.unsqueeze(-1), subjects, "bilinear", origins, labels, owner).squeeze(-1)


def stitch_subjects(original, detail_imgs, mask, subjects, labels=None, blend_overlap=1, filter="bilinear"):
    """The detailed crops `detail_imgs` [S * F, oh, ow, C] (subject-major, as crop_subjects stacks them) back into `original`
    [F, H, W, C].  The result is the composition of `stitch` in subject order, frame by frame:  out_0 = original,
    out_{s+1}[f] = stitch(out_s[f], detail[s * F + f], mask_s[f], window (s, f)),  bit for bit -- windows of different subjects
    may overlap, so the order counts -- computed as one copy of the frames and then, per subject, all frames' windows in one
    launch, in place."""
    _check_filter(filter)
    k = blend_overlap
    if not isinstance(k, int) or k < 1 or k > 51 or k % 2 == 0:
        raise ValueError(f"blend_overlap must be an odd integer in [1, 51], got {k!r}")
    orig = _as_f32c(_hip(original, "original"))
    det = _as_f32c(_hip(detail_imgs, "detail_imgs").to(orig.device))
    if orig.ndim != 4 or det.ndim != 4:
        raise ValueError("original and detail_imgs must be [B, H, W, C]")
    frames, H, W, c = orig.shape
    g, dev = subjects, orig.device
    _check_subjects(g, labels, frames, H, W)
    want = (g.subjects * frames, g.oh, g.ow, c)
    if tuple(det.shape) != want:
        raise ValueError(f"detail_imgs must be {want}, got {tuple(det.shape)}")
    m = _as_f32c(_frame_mask(mask, frames, H, W).to(dev))
    if g.resampled:
        det = detail._resample(det, Region(0, 0, g.oh, g.ow, g.h, g.w, g.oh, g.ow), filter)
    origins = _origins(g, dev)
    out = torch.empty_like(orig)
    d = _cabi.LpDetailStitchSubjectsDesc(frames, H, W, c, g.subjects, g.h, g.w, k, 0, 0, origins.data_ptr(), m.data_ptr(),
                                         orig.data_ptr(), det.data_ptr(), out.data_ptr())
    if labels is not None:
        owner = _owner_table(g.members, dev)
        d.labels, d.owner, d.owner_len = labels.data_ptr(), owner.data_ptr(), owner.numel()
    with torch.cuda.device(dev):
        _cabi.check(_cabi.load().lp_detail_stitch_subjects(ctypes.byref(d), raw_stream(dev)), "lp_detail_stitch_subjects")
    return out
