#!/usr/bin/env python3
"""Video shot detect benchmark (lanpaint_amd.shots on the HIP device): one JSON line.

The `clip` (81 frames of 1280 x 720 x 3) and `square` (16 frames of 1024 x 1024 x 3) workloads of scripts/bench_temporal_fill.py
with a hard cut put in: the second half of the clip is the first half's frames mirrored top to bottom and darkened.  Defaults
(threshold 16, hist 30, ratio 200, window 4, level 2, search 2).  Everything is already on the device.

    whole      shots.detect_shots against three things on the same clip in the same process, alternately: propagate.luma_pyramids
               alone at the same level (the cost that was there before), temporal_fill.temporal_fill, and the same rule in torch
               operators.  featurebench.wall, the median of `iters` runs and their min..max, and the ratios.
               featurebench.events around the call as well.
    split      between two device events (`reps` calls back to back): the pyramids, the measuring entry (two clears, the launch for
               all frames, the fold), the deciding launch.
    torch      the same rule in torch operators on the same device, on the whole clip, compared element by element: the elements
               of `score` and of `shot` that differ.
    shots      the ranges found (the one device -> host read), and what the cut's pair and the largest other pair scored.

    python scripts/bench_shots.py [--iters 5] [--warmup 1] [--case clip]
    python scripts/bench_shots.py --job whole --case clip --iters 3       # the body of a kernel-trace run
"""
from __future__ import annotations

import featurebench as fb

import bench_propagate as single  # the luma and the pyramid in torch
import bench_temporal_fill as fill  # the workloads

LEVEL, SEARCH, RATIO, WINDOW = 2, 2, 200, 4


def make_job(case, dev):
    """bench_temporal_fill's clip with a hard cut in the middle."""
    job = fill.make_job(case, dev)
    images = job["images"]
    k = images.shape[0] // 2
    images[k:] = images[:images.shape[0] - k].flip(1) * 0.5
    job["cut"] = k
    return job


# ---- the same rule in torch operators ----------------------------------------------------------------------------------------------------
def torch_scores(images, level=LEVEL, search=SEARCH):
    import torch
    import torch.nn.functional as Fn
    Y = single.torch_luma(images)
    Y = torch.stack([single._pyr(Y[f], level + 1, True)[level] for f in range(Y.shape[0])])
    F, h, w = Y.shape
    ys, xs = torch.arange(h, device=Y.device), torch.arange(w, device=Y.device)
    best = None
    for dy in range(-search, search + 1):
        for dx in range(-search, search + 1):
            moved = Y[1:][:, (ys + dy).clamp(0, h - 1)][:, :, (xs + dx).clamp(0, w - 1)]
            diff = Fn.pad((Y[:-1] - moved).abs(), (0, -w % 8, 0, -h % 8))
            sad = diff.view(F - 1, diff.shape[1] // 8, 8, diff.shape[2] // 8, 8).sum(dim=(2, 4))
            best = sad if best is None else torch.minimum(best, sad)
    frame = torch.arange(F, device=Y.device).view(F, 1, 1)
    hist = torch.bincount(((Y >> 2) + 64 * frame).flatten(), minlength=64 * F).view(F, 64)
    return torch.stack([best.sum(dim=(1, 2)), (hist[1:] - hist[:-1]).abs().sum(dim=1)], dim=1), h * w


def torch_decide(score, n, threshold, hist, ratio=RATIO, window=WINDOW):
    import torch
    A, B = score[:, 0], score[:, 1]
    ok = (A >= threshold * n) & (100 * B >= hist * 2 * n)
    for k in range(1, min(window, len(A) - 1) + 1):
        ok[k:] &= 100 * A[k:] >= ratio * A[:-k]
        ok[:-k] &= 100 * A[:-k] >= ratio * A[k:]
    return torch.cat([torch.zeros(1, dtype=torch.int64, device=score.device), ok.long().cumsum(0)]).int()


def torch_detect(images, threshold, hist):
    score, n = torch_scores(images)
    return torch_decide(score, n, threshold, hist), score


# ---- measurements ---------------------------------------------------------------------------------------------------------------------------
def measure(job, iters, warmup, reps):
    import torch
    from lanpaint_amd import _cabi, propagate, shots, temporal_fill as tf
    F, H, W = job["shape"]
    images, masks = job["images"], job["masks"]
    T, HI = shots.THRESHOLD, shots.HIST
    new = lambda: shots.detect_shots(images, T, HI, RATIO, WINDOW, LEVEL, SEARCH)                        # noqa: E731
    pyramids = lambda: propagate.luma_pyramids(images, LEVEL + 1)                                         # noqa: E731
    old = lambda: tf.temporal_fill(images, masks, fill.LEVELS, fill.SEARCH, fill.SMOOTH, 0)              # noqa: E731
    eager = lambda: torch_detect(images, T, HI)                                                           # noqa: E731
    shot, score = new()
    again = fb.differing(new(), (shot, score))
    t_shot, t_score = eager()
    from_torch = {"score": fb.differing(t_score, score), "shot": fb.differing(t_shot, shot)}
    ranges = shots.shot_ranges(shot)
    h, w = _cabi.prop_level_shape(H, W, LEVEL)
    n = h * w
    pyr = pyramids()
    off, stride = _cabi.prop_level_offset(H, W, LEVEL), pyr.shape[1]
    out = torch.empty((F - 1, 2), dtype=torch.int64, device=images.device)
    alone = lambda: shots.measure_planes(pyr[0, off:], stride, F, h, w, SEARCH, out)                      # noqa: E731
    decide = lambda: shots.shot_decide(score, n, T, HI, RATIO, WINDOW)                                   # noqa: E731
    fb.untimed(lambda: (new(), pyramids(), old(), eager(), alone(), decide()), warmup)
    med = fb.median
    # alternating: they share whatever else the host does
    s = fb.series([("new", new, fb.wall), ("pyramids", pyramids, fb.wall), ("old", old, fb.wall), ("torch", eager, fb.wall), ("events", new)],
                  iters, 0)
    new_ms, pyr_ms, old_ms, torch_ms, evs = s.values()
    A = score[:, 0].double() / n
    share = 50.0 * score[:, 1].double() / n
    others = torch.ones(F - 1, dtype=torch.bool, device=images.device)
    others[job["cut"] - 1] = False
    return {"case": job["case"], "frames_height_width": [F, H, W], "plane": [h, w], "threshold": T, "hist": HI, "ratio": RATIO,
            "window": WINDOW, "level": LEVEL, "search": SEARCH, "cut_at": job["cut"], "ranges": ranges,
            "cut_pair": {"A_over_N": round(float(A[job["cut"] - 1]), 2), "share_percent": round(float(share[job["cut"] - 1]), 1)},
            "other_pairs_max": {"A_over_N": round(float(A[others].max()), 2), "share_percent": round(float(share[others].max()), 1)},
            "detect_wall_ms": round(med(new_ms), 3), "detect_wall_min_max_ms": fb.summary(new_ms, 3)[1],
            "detect_events_ms": round(med(evs), 3), "ms_per_frame": round(med(new_ms) / F, 4),
            "pyramids_wall_ms": round(med(pyr_ms), 3), "pyramids_wall_min_max_ms": fb.summary(pyr_ms, 3)[1],
            "detect_over_pyramids": round(med(new_ms) / med(pyr_ms), 2),
            "fill_wall_ms": round(med(old_ms), 3), "fill_wall_min_max_ms": fb.summary(old_ms, 3)[1],
            "detect_over_fill": round(med(new_ms) / med(old_ms), 3),
            "torch_wall_ms": round(med(torch_ms), 3), "torch_over_detect": round(med(torch_ms) / med(new_ms), 1),
            "elements_differing_from_torch": from_torch, "elements_differing_between_two_calls": again,
            "stage_reps": reps,
            "split_ms": {"pyramids": round(fb.events(pyramids, reps), 4), "measure_entry": round(fb.events(alone, reps), 4),
                         "decide_launch": round(fb.events(decide, reps), 4)}}


def main():
    ap = fb.parser(single.CASES, ("whole",), iters=5, warmup=1)
    ap.add_argument("--reps", type=int, default=50, help="back-to-back calls per stage timing")
    a = ap.parse_args()
    dev = fb.device()
    import torch
    from lanpaint_amd import shots
    results = []
    for case in ((a.case,) if a.case else tuple(single.CASES)):
        job = make_job(case, dev)
        if a.job:
            fb.untimed(lambda: shots.detect_shots(job["images"]), a.warmup + a.iters)
        else:
            results.append(measure(job, a.iters, a.warmup, a.reps))
        del job
        torch.cuda.empty_cache()
    if not a.job:
        fb.emit("video_shot_detect", a, results)


if __name__ == "__main__":
    main()
