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

import torch

from . import _cabi, detail
from ._hostcall import launch, mask3, require_hip
from ._util import _as_f32c
from .detail import Subjects, _check_subjects         # Subjects is defined beside its siblings and is this module's to export


def _frame_mask(mask, frames, H, W):
    """The mask as [frames, H, W]: one plane per image."""
    m = mask3(mask if torch.is_tensor(mask) else require_hip(mask, "mask", __name__))
    if m.shape[0] == 1 and frames > 1:
        raise ValueError(f"the subjects form needs one mask plane per image, got one plane for {frames} images: a mask that "
                         "stands still is served by the region nodes (LanPaint_DetailerCropRegions)")
    if m.shape[0] != frames or tuple(m.shape[1:]) != (H, W):
        raise ValueError(f"mask shape {tuple(mask.shape)} does not match {frames} images of {H}x{W}")
    return require_hip(m, "mask", __name__)


def mask_components_frames(mask):
    """26-connected components of `mask > 0.5` in (f, y, x) of a HIP mask [F, H, W] (or [H, W], one frame), no union over
    planes: (labels int32 [F, H, W] on the device, n, table).  Labels run 1..n in raster order of each component's first voxel,
    0 is the background (scipy.ndimage.label with a 3 x 3 x 3 structure of ones); table[id - 1] = (f0, f1, r0, r1, c0, c1,
    volume), bounds inclusive, for id = 1..min(n, LP_DETAIL_MAX_COMPONENTS).  Reads the table back from the device: the first of
    a job's two reads."""
    return detail._components(mask, "lp_mask_components_frames", 7, volume=True)


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
        detail._merge_smallest_union(boxes, members)
    return tuple(members)


def subject_boxes(labels, members):
    """One bounding box per (subject, frame): boxes[s][f] = (row_min, row_max, col_min, col_max), inclusive, over the voxels of
    frame f whose label is one of members[s]; (H, -1, W, -1) for a frame the subject is absent from.  One launch
    (lp_subject_boxes); reads the [subjects, frames, 4] table back: the second of a job's two reads."""
    require_hip(labels, "labels", __name__)
    if labels.ndim != 3:
        raise ValueError(f"labels must be [F, H, W], got {tuple(labels.shape)}")
    frames, h, w = labels.shape
    detail._check_labels(labels, frames, h, w)
    members = detail._check_members(members)
    dev = labels.device
    owner = detail._owner_table(members, dev)
    boxes = torch.empty((len(members), frames, 4), dtype=torch.int32, device=dev)
    launch("lp_subject_boxes", dev, labels.data_ptr(), frames, h, w, owner.data_ptr(), owner.numel(), len(members),
           boxes.data_ptr())
    return tuple(tuple(tuple(row) for row in sub) for sub in boxes.cpu().tolist())


def plan_subjects(members, boxes, H, W, context=1.0, padding=0, multiple_of=8, target=0, smooth=1):
    """The module docstring's size, path and result steps: `members` from group_subjects, boxes[s][f] = (r0, r1, c0, c1)
    inclusive from subject_boxes, an absent frame as lp_subject_boxes marks it (r1 < r0) -> Subjects."""
    members = detail._check_members(members)
    H, W, c1000, padding, m, target = detail._plan_args(H, W, context, padding, multiple_of, target)
    smooth = detail._check_smooth(smooth)
    boxes = [[tuple(int(v) for v in box) for box in sub] for sub in boxes]
    frames = len(boxes[0]) if boxes else 0
    if len(boxes) != len(members) or frames < 1 or any(len(sub) != frames for sub in boxes) or \
            any(len(box) != 4 for sub in boxes for box in sub):
        raise ValueError(f"one row of boxes per subject and one box of four integers per frame are required: got {len(boxes)} "
                         f"rows for {len(members)} subjects")
    paths = []
    for s, sub in enumerate(boxes):
        paths.append(detail._box_spans(sub, H, W, lambda f: f"subject {s}, frame {f}: box"))
        if all(span is None for span in paths[-1][0]):
            raise ValueError(f"subject {s} is in no frame: the mask is empty in every frame of it, there is no region to detail")
    h = detail._track_size(max(sp[1] - sp[0] + 1 for rs, _ in paths for sp in rs if sp is not None), H, c1000, padding, m)
    w = detail._track_size(max(sp[1] - sp[0] + 1 for _, cs in paths for sp in cs if sp is not None), W, c1000, padding, m)
    origins = []
    for rs, cs in paths:
        ys, _ = detail._track_axis(rs, H, c1000, padding, m, smooth, h)
        xs, _ = detail._track_axis(cs, W, c1000, padding, m, smooth, w)
        origins.extend(zip(ys, xs))
    oh, ow = detail._working_size(h, w, m, target)
    return Subjects(H, W, h, w, oh, ow, tuple(origins), frames, members)


def crop_subjects(image, mask, subjects, labels=None, filter="bilinear"):
    """crop_resample for every (subject, frame) at once: (image [S * F, oh, ow, C], mask [S * F, oh, ow] or None),
    subject-major, so the stack is one sampler batch: entry s * F + f is frame f cut at `subjects.window(s, f)`.  Subject s's
    mask is frame f's with the components of other subjects -- and those min_area dropped -- set to 0 (`labels` from
    mask_components_frames; None: the mask as it is); values at or below 0.5 are nobody's and stay."""
    detail._check_filter(filter)
    img = _as_f32c(require_hip(image, "image", __name__))
    if img.ndim != 4:
        raise ValueError(f"image must be [B, H, W, C], got {tuple(image.shape)}")
    frames, H, W = img.shape[0], img.shape[1], img.shape[2]
    _check_subjects(subjects, labels, frames, H, W)
    origins = detail._origins_table(subjects, img.device)
    out = detail._resample(img, subjects, filter, origins)
    if mask is None:
        return out, None
    m = _as_f32c(_frame_mask(mask, frames, H, W).to(img.device))
    owner = None if labels is None else detail._owner_table(subjects.members, img.device)
    return out, detail._resample(m.unsqueeze(-1), subjects, "bilinear", origins, labels, owner).squeeze(-1)


def stitch_subjects(original, detail_imgs, mask, subjects, labels=None, blend_overlap=1, filter="bilinear"):
    """The detailed crops `detail_imgs` [S * F, oh, ow, C] (subject-major, as crop_subjects stacks them) back into `original`
    [F, H, W, C].  The result is the composition of `stitch` in subject order, frame by frame:  out_0 = original,
    out_{s+1}[f] = stitch(out_s[f], detail[s * F + f], mask_s[f], window (s, f)),  bit for bit -- windows of different subjects
    may overlap, so the order counts -- computed as one copy of the frames and then, per subject, all frames' windows in one
    launch, in place."""
    orig, det, m, frames, H, W, c = detail._stitch_inputs(original, detail_imgs, mask, subjects, blend_overlap, filter, labels,
                                                          frame_mask=_frame_mask)
    g, dev = subjects, orig.device
    origins = detail._origins_table(g, dev)
    out = torch.empty_like(orig)
    d = _cabi.LpDetailStitchSubjectsDesc(frames, H, W, c, g.subjects, g.h, g.w, blend_overlap, 0, 0, origins.data_ptr(),
                                         m.data_ptr(), orig.data_ptr(), det.data_ptr(), out.data_ptr())
    if labels is not None:
        owner = detail._owner_table(g.members, dev)
        d.labels, d.owner, d.owner_len = labels.data_ptr(), owner.data_ptr(), owner.numel()
    launch("lp_detail_stitch_subjects", dev, ctypes.byref(d))
    return out
