"""The subjects rule of lanpaint_amd/detail_subjects.py restated plainly with numpy / scipy, and the arbiters of the per-subject
Detailer's device tests: the space-time labelling (scipy.ndimage.label with a 3 x 3 x 3 structure of ones), the boxes per
(subject, frame), subject s's erased mask built in torch from the label volume, and the composed stitch with torch CPU
operators.  Nothing here touches a device or shares a helper with the package's planners."""
import numpy as np
import torch
from scipy import ndimage

from tests import detail_ref


# ---- labelling -----------------------------------------------------------------------------------------------------------------
def label_frames_ref(S):
    """S bool [F, H, W] -> (labels int32 [F, H, W], n, table int64 [n, 7] = (f0, f1, r0, r1, c0, c1, volume)).  scipy numbers
    components in raster order of their first voxel; asserted here, since the device's labels are defined that way."""
    S = np.asarray(S, bool)
    labels, n = ndimage.label(S, np.ones((3, 3, 3), np.int32))
    labels = labels.astype(np.int32)
    table = np.zeros((n, 7), np.int64)
    if n:
        flat = labels.ravel()
        first = np.full(n + 1, flat.size, np.int64)
        np.minimum.at(first, flat, np.arange(flat.size))
        assert np.all(np.diff(first[1:]) > 0), "scipy's labels are not in raster order of first voxel"
        f, y, x = np.nonzero(S)
        lab = labels[f, y, x] - 1
        for col, v in ((0, f), (2, y), (4, x)):
            lo = np.full(n, np.iinfo(np.int64).max, np.int64)
            hi = np.full(n, -1, np.int64)
            np.minimum.at(lo, lab, v)
            np.maximum.at(hi, lab, v)
            table[:, col], table[:, col + 1] = lo, hi
        table[:, 6] = np.bincount(lab, minlength=n)
    return labels, int(n), table


def subject_boxes_ref(labels, members):
    """labels int [F, H, W], members: tuple of label tuples -> int64 [S, F, 4] = (r0, r1, c0, c1), (H, -1, W, -1) when absent."""
    labels = np.asarray(labels)
    F, H, W = labels.shape
    out = np.zeros((len(members), F, 4), np.int64)
    for s, mem in enumerate(members):
        own = np.isin(labels, np.asarray(mem))
        for f in range(F):
            ys, xs = np.nonzero(own[f])
            out[s, f] = (ys.min(), ys.max(), xs.min(), xs.max()) if ys.size else (H, -1, W, -1)
    return out


# ---- the rule ----------------------------------------------------------------------------------------------------------------
def group_subjects_ref(n, table, min_area, max_subjects, cap):
    if n > cap:
        return (tuple(range(1, n + 1)),)
    groups = []                                                  # [box of six, members]
    for label in range(1, n + 1):
        f0, f1, r0, r1, c0, c1, volume = (int(v) for v in table[label - 1])
        if volume >= min_area * (f1 - f0 + 1):
            groups.append([[f0, f1, r0, r1, c0, c1], [label]])
    if not groups:
        raise ValueError("nothing kept")
    while len(groups) > max_subjects:
        best = None
        for i in range(len(groups)):
            for j in range(i + 1, len(groups)):
                a, b = groups[i][0], groups[j][0]
                product = 1
                for axis in range(3):
                    product *= max(a[2 * axis + 1], b[2 * axis + 1]) - min(a[2 * axis], b[2 * axis]) + 1
                if best is None or product < best[0]:            # strict: ties keep the lowest i, then the lowest j
                    best = (product, i, j)
        _, i, j = best
        a, b = groups[i][0], groups[j][0]
        groups[i] = [[min(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), max(a[3], b[3]), min(a[4], b[4]), max(a[5], b[5])],
                     sorted(groups[i][1] + groups[j][1])]
        del groups[j]
    return tuple(tuple(g[1]) for g in groups)


def _path_ref(spans, N, n, k):
    """fill, smooth, contain, clamp of the track rule on one axis with the window size n given."""
    F = len(spans)
    s = [None if sp is None else sp[0] + sp[1] + 1 for sp in spans]
    filled = list(s)
    for f in range(F):
        if s[f] is not None:
            continue
        p = f - 1
        while p >= 0 and s[p] is None:
            p -= 1
        q = f + 1
        while q < F and s[q] is None:
            q += 1
        if p >= 0 and q < F:
            filled[f] = s[p] + ((s[q] - s[p]) * (f - p)) // (q - p)
        else:
            filled[f] = s[p] if p >= 0 else s[q]
    los = []
    for f in range(F):
        total = 0
        for j in range(-(k // 2), k // 2 + 1):
            total += filled[min(max(f + j, 0), F - 1)]
        lo = (total - k * n) // (2 * k)
        if spans[f] is not None:
            lo = min(lo, spans[f][0])
            lo = max(lo, spans[f][1] + 1 - n)
        los.append(min(max(lo, 0), N - n))
    return los


def _size_ref(side, N, c, padding, M):
    g = padding + ((c - 1000) * side + 1999) // 2000
    n = min(side + 2 * g, N)
    need = ((n + M - 1) // M) * M
    return need if need <= N else n


def plan_subjects_ref(boxes, H, W, context, padding, M, target, smooth):
    """boxes [S][F] of (r0, r1, c0, c1) -> (H, W, h, w, oh, ow, origins) with origins subject-major, plain integers."""
    c = int(round(context * 1000))
    side_h = side_w = 0
    for sub in boxes:
        for r0, r1, c0, c1 in sub:
            if r1 >= r0 and c1 >= c0:
                side_h, side_w = max(side_h, r1 - r0 + 1), max(side_w, c1 - c0 + 1)
    h, w = _size_ref(side_h, H, c, padding, M), _size_ref(side_w, W, c, padding, M)
    origins = []
    for sub in boxes:
        rows = [None if (r1 < r0 or c1 < c0) else (r0, r1) for r0, r1, c0, c1 in sub]
        cols = [None if (r1 < r0 or c1 < c0) else (c0, c1) for r0, r1, c0, c1 in sub]
        origins.extend(zip(_path_ref(rows, H, h, smooth), _path_ref(cols, W, w, smooth)))
    if target <= 0:
        oh, ow = h, w
    else:
        L = max(h, w)
        oh = max(1, (2 * h * target + L * M) // (2 * L * M)) * M
        ow = max(1, (2 * w * target + L * M) // (2 * L * M)) * M
    return H, W, h, w, oh, ow, tuple(origins)


# ---- subject s's mask, the composed stitch --------------------------------------------------------------------------------------
def subject_mask(mask, labels, members):
    """mask [F, H, W] torch CPU with foreign components erased frame by frame: 0 where labels != 0 and the label is not in
    `members`; label 0 (values at or below 0.5) stays."""
    lab = torch.as_tensor(np.asarray(labels))
    foreign = (lab != 0) & ~torch.isin(lab, torch.tensor(list(members), dtype=lab.dtype))
    return torch.where(foreign, torch.zeros((), dtype=mask.dtype), mask)


def stitch_subjects_ref(original, detail_imgs, mask, subjects, labels, k, filter):
    """detail_ref.stitch_ref composed in subject order, frame by frame, with the CPU-built subject masks."""
    F = original.shape[0]
    out = original.clone()
    for s in range(subjects.subjects):
        ms = subject_mask(mask, labels, subjects.members[s])
        for f in range(F):
            out[f:f + 1] = detail_ref.stitch_ref(out[f:f + 1], detail_imgs[s * F + f:s * F + f + 1], ms[f:f + 1],
                                                 subjects.window(s, f), k, filter)
    return out


def cover_count(subjects):
    """[F, H, W] int: how many windows cover each pixel of each frame."""
    c = np.zeros((subjects.frames, subjects.H, subjects.W), np.int64)
    for i, (y0, x0) in enumerate(subjects.origins):
        c[i % subjects.frames, y0:y0 + subjects.h, x0:x0 + subjects.w] += 1
    return c
