#!/usr/bin/env python3
"""Anchored video mask propagate from several keyframes (lanpaint_amd.propagate_keys_anchored on the HIP device): one JSON line.

The `clip` (81 frames of 1280 x 720 x 3) and `square` (16 frames of 1024 x 1024 x 3) workloads of scripts/bench_propagate.py at
the default parameters and anchor 2, the true disc painted on the first and the last frame.  Everything is already on the device,
and everything that is compared runs in this one process, alternating.

    whole      propagate_keys_anchored.propagate_keys_anchored against propagate_keys.propagate_keys on the same input,
               featurebench.wall: the median of `iters` runs each, their min..max and the ratio.
    launches   counted by wrapping the modules' launch(): the batched entry calls of both, the dependent steps.
    edt        stabilize.signed_d2 on the gap's two stacks alone, featurebench.events, and its share of the anchored call.
    batch      lp_prop_match_batch in its warped-key form with 2 and 32 jobs against as many single lp_prop_anchor_match launches
               on the same buffers, featurebench.events over `reps` calls back to back, alternating over `rounds`: the median
               ms per call of each, and whether the two gave the same elements.
    drift      the lowest per-frame IoU with the true disc of both calls on scripts/bench_propagate_anchored.py's sub-pixel clip
               of the same size, keys on both ends (--no-drift skips it).

    python scripts/bench_propagate_keys_anchored.py [--iters 5] [--warmup 1] [--case clip] [--reps 50] [--rounds 7]
    python scripts/bench_propagate_keys_anchored.py --job whole --case clip        # the body of a kernel-trace run
"""
from __future__ import annotations

import featurebench as fb

import bench_propagate as single
import bench_propagate_anchored as anchored
import bench_propagate_keys as keyed

LEVELS, SEARCH, SMOOTH, ANCHOR = single.LEVELS, single.SEARCH, single.SMOOTH, anchored.ANCHOR


def batch_times(job, jobs, reps, rounds):
    """The batched warped match with `jobs` jobs and as many single launches, on the first steps' buffers of `jobs` chains (every
    chain the clip's first step; the work of a job does not depend on which frame it is): (batched ms, singles ms, same)."""
    import ctypes

    import torch
    from lanpaint_amd import _cabi, propagate, propagate_anchored as pa, propagate_keys as pk
    from lanpaint_amd._hostcall import launch
    F, H, W = job["shape"]
    dev = job["images"].device
    pyr = propagate.luma_pyramids(job["images"][:2], LEVELS)
    mpyr, _ = propagate.key_mask(job["mask"], LEVELS)
    step = propagate.Step(H, W, LEVELS, SEARCH, SMOOTH, dev, rematch=(pa.anchor_field, ANCHOR, SMOOTH))
    vec = step.field_of(pyr[0], pyr[1], mpyr)
    key_bits = propagate.level_view(mpyr, H, W, 0)[0]
    rows, planes, outs = [], [], []
    for _ in range(jobs):                                              # a chain's own positions and bits per job, as Chains holds them
        pos, _, bits = propagate.advance(vec, None, key_bits, LEVELS, torch.empty_like(step.raw_pos), step.code, torch.empty_like(step.raw_mpyr))
        rows.append((pyr[0], pyr[1], bits, pos))
        planes.append((pos, propagate.level_view(pyr[1:2], H, W, 0)[0], propagate.level_view(pyr[0:1], H, W, 0)[0],
                       propagate.level_view(bits, H, W, 0)[0]))
        outs.append((torch.empty_like(step.raw[0]), torch.empty_like(step.valid[0])))
    b_outs = [(torch.empty_like(step.raw[0]), torch.empty_like(step.valid[0])) for _ in range(jobs)]
    table = pk.job_table([(*r, *o) for r, o in zip(rows, b_outs)], "bench")
    d = _cabi.LpPropMatchBatchDesc(H, W, LEVELS, 0, ANCHOR, SMOOTH, jobs, _cabi.LP_PROP_MATCH_WARPED_KEY, table.ctypes.data)
    batched_fn = lambda: launch("lp_prop_match_batch", dev, ctypes.byref(d))                                # noqa: E731
    singles_fn = lambda: [pa.anchor_field(*p, ANCHOR, SMOOTH, *o) for p, o in zip(planes, outs)]           # noqa: E731
    batched_ms, singles_ms = fb.series([("batched", batched_fn), ("singles", singles_fn)], rounds, 1, timer=lambda f: fb.events(f, reps)).values()
    same = all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(outs, b_outs))
    return fb.median(batched_ms), fb.median(singles_ms), bool(same)


def drift(case, dev):
    """The lowest per-frame IoU of the two calls on the sub-pixel clip, the true disc painted on both ends."""
    from lanpaint_amd import propagate_keys as pk, propagate_keys_anchored as pka
    images, truth = anchored.subpixel_job(case, dev)
    F = truth.shape[0]
    keys, masks = [0, F - 1], truth[[0, F - 1]].float()
    worst = lambda out: round(min(anchored.iou(out[t] >= 0.5, truth[t]) for t in range(F)), 4)              # noqa: E731
    return {"anchored_lowest_iou": worst(pka.propagate_keys_anchored(images, masks, keys, LEVELS, SEARCH, SMOOTH, ANCHOR)),
            "keys_lowest_iou": worst(pk.propagate_keys(images, masks, keys, LEVELS, SEARCH, SMOOTH))}


def measure(job, iters, warmup, reps, rounds):
    from lanpaint_amd import propagate_keys as pk, propagate_keys_anchored as pka, stabilize
    F, H, W = job["shape"]
    keys = [0, F - 1]
    masks = keyed.painted(job, keys)
    new = lambda: pka.propagate_keys_anchored(job["images"], masks, keys, LEVELS, SEARCH, SMOOTH, ANCHOR)    # noqa: E731
    old = lambda: pk.propagate_keys(job["images"], masks, keys, LEVELS, SEARCH, SMOOTH)                     # noqa: E731
    names_new, names_old = fb.count_launches(new, pk), fb.count_launches(old, pk)      # pka launches through pk's Chains
    got = new()
    again = fb.differing(new(), got)
    off = fb.differing(pka.propagate_keys_anchored(job["images"], masks, keys, LEVELS, SEARCH, SMOOTH, 0), old())
    moved = fb.differing(got, old())
    edt_of = lambda: [stabilize.signed_d2(got[1:F - 1]) for _ in range(2)]                                   # noqa: E731
    # alternating: the two share whatever else the host does
    fb.untimed(lambda: (new(), old()), warmup)
    new_ms, old_ms, edts = fb.series([("new", new, fb.wall), ("old", old, fb.wall), ("edt", edt_of)], iters, 0).values()
    del got
    med = fb.median
    plan = pk.chain_plan(F, keys)
    out = {"case": job["case"], "key_frames": keys, "frames_height_width": [F, H, W], "levels": LEVELS, "search": SEARCH, "smooth": SMOOTH,
           "anchor": ANCHOR,
           "anchored_wall_ms": round(med(new_ms), 3), "anchored_wall_min_max_ms": fb.summary(new_ms, 3)[1],
           "keys_wall_ms": round(med(old_ms), 3), "keys_wall_min_max_ms": fb.summary(old_ms, 3)[1],
           "anchored_over_keys": round(med(new_ms) / med(old_ms), 3),
           "chains": len(plan), "dependent_steps": max(c[3] for c in plan),
           "batched_entry_calls": [sum(n.endswith("_batch") for n in names_new), sum(n.endswith("_batch") for n in names_old)],
           "entry_calls_by_name": {k: names_new.count(k) for k in sorted(set(names_new))},
           "edt_ms": round(med(edts), 3), "edt_share": round(med(edts) / med(new_ms), 3),
           "elements_differing_between_two_calls": again, "elements_differing_from_keys_at_anchor_0": off,
           "elements_differing_from_keys": moved, "launch_reps_rounds": [reps, rounds]}
    for jobs in (2, 32):
        b, s, same = batch_times(job, jobs, reps, rounds)
        out[f"batch_{jobs}_jobs"] = {"batched_ms": round(b, 5), "singles_ms": round(s, 5), "singles_over_batched": round(s / b, 3),
                                     "same_elements": same}
    return out


def main():
    ap = fb.parser(single.CASES, ("whole",), iters=5, warmup=1)
    ap.add_argument("--reps", type=int, default=50, help="back-to-back calls per launch timing")
    ap.add_argument("--rounds", type=int, default=7, help="alternating launch timings, of which the median is taken")
    ap.add_argument("--no-drift", action="store_true", help="skip the sub-pixel clip's IoU")
    a = ap.parse_args()
    dev = fb.device()
    import torch
    from lanpaint_amd import propagate_keys_anchored as pka
    results = []
    for case in ((a.case,) if a.case else tuple(single.CASES)):
        job = single.make_job(case, dev)
        F = job["shape"][0]
        if a.job:
            masks = keyed.painted(job, [0, F - 1])
            fb.untimed(lambda: pka.propagate_keys_anchored(job["images"], masks, [0, F - 1], LEVELS, SEARCH, SMOOTH, ANCHOR), a.warmup + a.iters)
        else:
            results.append(measure(job, a.iters, a.warmup, a.reps, a.rounds))
            del job
            torch.cuda.empty_cache()
            if not a.no_drift:
                results[-1]["subpixel_clip"] = drift(case, dev)
        torch.cuda.empty_cache()
    if not a.job:
        fb.emit("mask_propagate_keys_anchored", a, results)


if __name__ == "__main__":
    main()
