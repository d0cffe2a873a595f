"""Arbiters of the per-region Detailer tests (tests/test_detail_regions_host.py, tests/test_gpu_detail_regions.py), numpy only:
connected-component labelling, the regions rule restated pair by pair, region i's mask and the composed stitch.  Nothing here
touches a device or needs scipy."""
import numpy as np
import torch

from lanpaint_amd import detail
from tests import detail_ref


def union_set(mask):
    """S of the labelling's definition: mask [planes, H, W], [H, W] (numpy or torch, CPU) -> bool [H, W], > 0.5 in any plane."""
    m = np.asarray(mask)
    return (m > np.float32(0.5)).reshape(-1, m.shape[-2], m.shape[-1]).any(0)


def label_ref(S):
    """Two-pass union-find labelling of bool [H, W] with 8-connectivity, over row runs: pass one gives every run a provisional
    id in raster order and unites it with the runs of the row above that it touches (columns overlap once either run is
    widened by one: the diagonal counts), always onto the smaller id; pass two ranks the roots.  A root is its component's
    first run in raster order, so labels run 1..n in raster order of each component's first pixel.
    Returns (labels int32 [H, W], n, table int64 [n, 5] = (r0, r1, c0, c1, area), boxes inclusive)."""
    S = np.asarray(S, bool)
    H, W = S.shape
    padded = np.zeros((H, W + 2), np.int8)
    padded[:, 1:-1] = S
    edges = np.diff(padded, axis=1)
    rows, starts = np.nonzero(edges == 1)                       # raster order
    ends = np.nonzero(edges == -1)[1]                           # exclusive
    n_runs = len(rows)
    parent = list(range(n_runs))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    first = np.searchsorted(rows, np.arange(H + 1))            # runs of row y: first[y] .. first[y + 1]
    rs, re = starts.tolist(), ends.tolist()
    for y in range(1, H):
        a, a_end, b, b_end = first[y - 1], first[y], first[y], first[y + 1]
        while a < a_end and b < b_end:
            if rs[a] <= re[b] and rs[b] <= re[a]:               # [s, e) widened by one on either side overlap
                ra, rb = find(a), find(b)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
            if re[a] <= re[b]:
                a += 1
            else:
                b += 1
    roots = np.array([find(a) for a in range(n_runs)], np.int64)
    is_root = roots == np.arange(n_runs)
    rank = np.cumsum(is_root)                                   # 1-based label of a root run
    run_label = rank[roots] if n_runs else np.zeros(0, np.int64)
    n = int(is_root.sum())
    lengths = ends - starts
    labels = np.zeros((H, W), np.int32)
    flat = np.repeat(rows * W + starts, lengths) + (np.arange(lengths.sum()) - np.repeat(np.cumsum(lengths) - lengths, lengths))
    labels.reshape(-1)[flat] = np.repeat(run_label, lengths)
    table = np.zeros((n, 5), np.int64)
    table[:, 0], table[:, 2] = H, W
    table[:, 1] = table[:, 3] = -1
    idx = run_label - 1
    np.minimum.at(table[:, 0], idx, rows)
    np.maximum.at(table[:, 1], idx, rows)
    np.minimum.at(table[:, 2], idx, starts)
    np.maximum.at(table[:, 3], idx, ends - 1)
    np.add.at(table[:, 4], idx, lengths)
    return labels, n, table


def components_of(S):
    """label_ref as lanpaint_amd.detail.mask_components returns it, without the device: (labels, n, table of tuples)."""
    labels, n, table = label_ref(S)
    return labels, n, tuple(tuple(int(v) for v in row) for row in table[:detail._cabi.LP_DETAIL_MAX_COMPONENTS])


# ---- the regions rule, restated as its text reads: every step searches every pair again ---------------------------------------
def plan_regions_ref(n, table, H, W, context, padding, m, target, min_area=1, max_regions=8):
    c1000 = int(round(float(context) * 1000))
    groups = [([r0, r1, c0, c1], [label]) for label, (r0, r1, c0, c1, area) in enumerate(table, 1) if area >= min_area]
    assert groups

    def window(box):
        return detail._plan_axis(box[0], box[1], H, c1000, padding, m) + detail._plan_axis(box[2], box[3], W, c1000, padding, m)

    def merge(i, j):
        (a, ma), (b, mb) = groups[i], groups[j]
        groups[i] = ([min(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), max(a[3], b[3])], sorted(ma + mb))
        del groups[j]
        groups.sort(key=lambda g: g[1][0])

    def close():
        while True:
            win = [window(g[0]) for g in groups]
            pair = next(((i, j) for i in range(len(groups)) for j in range(i + 1, len(groups))
                         if win[i][0] < win[j][0] + win[j][1] and win[j][0] < win[i][0] + win[i][1]
                         and win[i][2] < win[j][2] + win[j][3] and win[j][2] < win[i][2] + win[i][3]), None)
            if pair is None:
                return
            merge(*pair)

    close()
    while len(groups) > max_regions:
        best = None
        for i in range(len(groups)):
            for j in range(i + 1, len(groups)):
                a, b = groups[i][0], groups[j][0]
                area = (max(a[1], b[1]) - min(a[0], b[0]) + 1) * (max(a[3], b[3]) - min(a[2], b[2]) + 1)
                if best is None or area < best[0]:
                    best = (area, i, j)
        merge(best[1], best[2])
        close()
    win = [window(g[0]) for g in groups]
    h, w = max(v[1] for v in win), max(v[3] for v in win)
    origins = []
    for y0, hi, x0, wi in win:
        y0 -= (h - hi) // 2
        x0 -= (w - wi) // 2
        origins.append((min(max(y0, 0), H - h), min(max(x0, 0), W - w)))
    oh, ow = h, w
    if target > 0:                                              # s * target / L to the nearest multiple of m, halves up
        long_side = max(h, w)
        oh = max(1, (2 * h * target + long_side * m) // (2 * long_side * m)) * m
        ow = max(1, (2 * w * target + long_side * m) // (2 * long_side * m)) * m
    return detail.Regions(H, W, h, w, oh, ow, tuple(origins), tuple(tuple(g[1]) for g in groups))


# ---- region i's mask, the composed stitch ------------------------------------------------------------------------------------
def region_mask(mask, labels, members):
    """mask [Bm, H, W] torch CPU with foreign components erased: 0 where labels != 0 and the label is not in `members`."""
    lab = torch.as_tensor(np.asarray(labels))
    foreign = (lab != 0) & ~torch.isin(lab, torch.tensor(list(members), dtype=lab.dtype))
    return torch.where(foreign.unsqueeze(0), torch.zeros((), dtype=mask.dtype), mask)


def stitch_regions_ref(original, detail_imgs, mask, regions, labels, k, filter):
    """detail_ref.stitch_ref composed in region order with the CPU-built region masks."""
    b = original.shape[0]
    out = original
    for i in range(len(regions)):
        out = detail_ref.stitch_ref(out, detail_imgs[i * b:(i + 1) * b], region_mask(mask, labels, regions.members[i]),
                                    regions.region(i), k, filter)
    return out


def cover_count(regions):
    """[H, W] int: how many windows cover each pixel."""
    c = np.zeros((regions.H, regions.W), np.int64)
    for y0, x0 in regions.origins:
        c[y0:y0 + regions.h, x0:x0 + regions.w] += 1
    return c
