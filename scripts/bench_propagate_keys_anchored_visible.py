#!/usr/bin/env python3
"""Anchored occlusion-aware video mask propagate from several keyframes (lanpaint_amd.propagate_keys_anchored_visible on the HIP
device): one JSON line.

The `clip` (81 frames of 1280 x 720 x 3) and `square` (16 frames of 1024 x 1024 x 3) workloads of scripts/bench_propagate.py at
the default parameters, anchor 2 and occlusion 16, the true disc painted on the first and the last frame.  Everything is already
on the device, and everything that is compared runs in this one process, alternating.

    whole      propagate_keys_anchored_visible against propagate_keys_visible, propagate_keys_anchored and propagate_keys on the
               same input, featurebench.wall: the median of `iters` runs each, their min..max and the three ratios.
    launches   counted by wrapping the modules' launch(): the batched entry calls of the four, the dependent steps.
    batch      lp_prop_match_batch in its gated form with 2 and 32 jobs against as many single lp_prop_anchor_match_gated
               launches on the same buffers, featurebench.events over `reps` calls back to back, alternating over `rounds`:
               the median ms per call of each, and whether the two gave the same elements.
    occluded   the whole-subject IoU (mask + hidden >= 0.5; worst frame and mean) of the new form, propagate_keys_visible and
               propagate_keys_anchored (hidden = 0) on scripts/bench_propagate_anchored.py's sub-pixel clip of the same size with
               a static textured bar of W / 20 columns in the subject's way, keys on both ends (--no-occluded skips it).

    python scripts/bench_propagate_keys_anchored_visible.py [--iters 5] [--warmup 1] [--case clip] [--reps 50] [--rounds 7]
    python scripts/bench_propagate_keys_anchored_visible.py --job whole --case clip        # the body of a kernel-trace run
"""
from __future__ import annotations

import featurebench as fb

import bench_propagate as single
import bench_propagate_anchored as anchored
import bench_propagate_keys as keyed

LEVELS, SEARCH, SMOOTH, ANCHOR, OCCLUSION = single.LEVELS, single.SEARCH, single.SMOOTH, anchored.ANCHOR, 16


def batch_times(job, jobs, reps, rounds):
    """The batched gated match with `jobs` jobs and as many single gated launches, on the first steps' buffers of `jobs` chains
    (every chain the clip's first step; the work of a job does not depend on which frame it is): (batched ms, singles ms, same)."""
    import ctypes

    import torch
    from lanpaint_amd import _cabi, propagate, propagate_anchored_visible as pav, propagate_keys as pk
    from lanpaint_amd._hostcall import launch
    F, H, W = job["shape"]
    dev = job["images"].device
    pyr = propagate.luma_pyramids(job["images"][:2], LEVELS)
    mpyr, _ = propagate.key_mask(job["mask"], LEVELS)
    step = propagate.Step(H, W, LEVELS, SEARCH, SMOOTH, dev, rematch=(pav.gated_anchor_field, ANCHOR, SMOOTH, OCCLUSION),
                          split=(pav.visible_flags, pav.occlude, OCCLUSION))
    vec = step.field_of(pyr[0], pyr[1], mpyr)
    key_bits = propagate.level_view(mpyr, H, W, 0)[0]
    rows, planes, outs = [], [], []
    for _ in range(jobs):                                              # a chain's own positions and bits per job, as Chains holds them
        pos, _, bits = propagate.advance(vec, None, key_bits, LEVELS, torch.empty_like(step.raw_pos), step.code, torch.empty_like(step.raw_mpyr))
        rows.append((pyr[0], pyr[1], bits, pos))
        planes.append((pos, propagate.level_view(pyr[1:2], H, W, 0)[0], propagate.level_view(pyr[0:1], H, W, 0)[0],
                       propagate.level_view(bits, H, W, 0)[0]))
        outs.append((torch.empty_like(step.raw[0]), torch.empty_like(step.valid[0]), torch.empty_like(step.gated)))
    b_outs = [(torch.empty_like(step.raw[0]), torch.empty_like(step.valid[0])) for _ in range(jobs)]
    table = pk.job_table([(*r, *o) for r, o in zip(rows, b_outs)], "bench")
    d = _cabi.LpPropMatchBatchDesc(H, W, LEVELS, 0, ANCHOR, SMOOTH, jobs, _cabi.LP_PROP_MATCH_GATED(OCCLUSION), table.ctypes.data)
    batched_fn = lambda: launch("lp_prop_match_batch", dev, ctypes.byref(d))                                            # noqa: E731
    singles_fn = lambda: [pav.gated_anchor_field(*p, ANCHOR, SMOOTH, OCCLUSION, *o) for p, o in zip(planes, outs)]     # noqa: E731
    batched_ms, singles_ms = fb.series([("batched", batched_fn), ("singles", singles_fn)], rounds, 1, timer=lambda f: fb.events(f, reps)).values()
    same = all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(outs, b_outs))
    return fb.median(batched_ms), fb.median(singles_ms), bool(same), [int(outs[0][2].sum()), int(outs[0][1].sum())]


def occluded(case, dev):
    """Whole-subject IoU [worst frame, mean] of the three several-keys forms on the sub-pixel clip with a static bar in the
    subject's way (the bar of scripts/bench_propagate_anchored_visible.py), the true disc painted on both ends."""
    import torch
    from lanpaint_amd import propagate_keys_anchored as pka, propagate_keys_anchored_visible as pkav, propagate_keys_visible as pkv
    images, truth = anchored.subpixel_job(case, dev)
    F, H, W = truth.shape
    x0 = int(0.3 * W + min(H, W) / 5 + 0.2 * W / 20)                   # just right of the disc on the first key frame
    g = torch.Generator(device="cpu").manual_seed(99)
    bar = torch.rand(H, W // 20, generator=g).to(dev)
    for ax in (0, 1):
        bar = (torch.roll(bar, -1, ax) + 2 * bar + torch.roll(bar, 1, ax)) / 4
    images[:, :, x0:x0 + W // 20, :] = ((bar - bar.min()) / (bar.max() - bar.min()))[None, :, :, None]
    keys, masks = [0, F - 1], truth[[0, F - 1]].float()

    def both(m, h=None):
        v = [anchored.iou(((m[t] + h[t]) if h is not None else m[t]) >= 0.5, truth[t]) for t in range(F)]
        return [round(min(v), 4), round(sum(v) / F, 4)]
    behind = max(float((truth[t, :, x0:x0 + W // 20]).sum()) / float(truth[t].sum()) for t in range(F))
    return {"bar_columns": [x0, x0 + W // 20], "largest_part_of_the_subject_behind_the_bar": round(behind, 3),
            "new_worst_mean_iou": both(*pkav.propagate_keys_anchored_visible(images, masks, keys, LEVELS, SEARCH, SMOOTH, ANCHOR, OCCLUSION)),
            "keys_visible_worst_mean_iou": both(*pkv.propagate_keys_visible(images, masks, keys, LEVELS, SEARCH, SMOOTH, OCCLUSION)),
            "keys_anchored_worst_mean_iou": both(pka.propagate_keys_anchored(images, masks, keys, LEVELS, SEARCH, SMOOTH, ANCHOR))}


def measure(job, iters, warmup, reps, rounds):
    from lanpaint_amd import (propagate_keys as pk, propagate_keys_anchored as pka, propagate_keys_anchored_visible as pkav,
                              propagate_keys_visible as pkv)
    F, H, W = job["shape"]
    keys = [0, F - 1]
    masks = keyed.painted(job, keys)
    images = job["images"]
    calls = {"new": lambda: pkav.propagate_keys_anchored_visible(images, masks, keys, LEVELS, SEARCH, SMOOTH, ANCHOR, OCCLUSION),
             "keys_visible": lambda: pkv.propagate_keys_visible(images, masks, keys, LEVELS, SEARCH, SMOOTH, OCCLUSION),
             "keys_anchored": lambda: pka.propagate_keys_anchored(images, masks, keys, LEVELS, SEARCH, SMOOTH, ANCHOR),
             "keys": lambda: pk.propagate_keys(images, masks, keys, LEVELS, SEARCH, SMOOTH)}
    names = {k: fb.count_launches(fn, pk) for k, fn in calls.items()}      # every form launches its steps through pk's Chains
    got = calls["new"]()
    again = fb.differing(calls["new"](), got)
    off = {"anchor_0": fb.differing(pkav.propagate_keys_anchored_visible(images, masks, keys, LEVELS, SEARCH, SMOOTH, 0, OCCLUSION),
                                    calls["keys_visible"]()),
           "occlusion_0": fb.differing(pkav.propagate_keys_anchored_visible(images, masks, keys, LEVELS, SEARCH, SMOOTH, ANCHOR, 0)[0],
                                       calls["keys_anchored"]())}
    del got
    ms = fb.series(list(calls.items()), iters, warmup, timer=fb.wall)    # alternating: the four share whatever else the host does
    med = fb.median
    plan = pk.chain_plan(F, keys)
    out = {"case": job["case"], "key_frames": keys, "frames_height_width": [F, H, W], "levels": LEVELS, "search": SEARCH, "smooth": SMOOTH,
           "anchor": ANCHOR, "occlusion": OCCLUSION, "chains": len(plan), "dependent_steps": max(c[3] for c in plan)}
    for k in calls:
        out[f"{k}_wall_ms"], out[f"{k}_wall_min_max_ms"] = fb.summary(ms[k], 3)
        out[f"{k}_batched_entry_calls"] = sum(n.endswith("_batch") for n in names[k])
    for k in ("keys_visible", "keys_anchored", "keys"):
        out[f"new_over_{k}"] = round(med(ms["new"]) / med(ms[k]), 3)
    out["entry_calls_by_name"] = {k: names["new"].count(k) for k in sorted(set(names["new"]))}
    out["elements_differing_between_two_calls"] = again
    out["elements_differing_on_the_off_routes"] = off
    out["launch_reps_rounds"] = [reps, rounds]
    for jobs in (2, 32):
        b, s, same, blocks = batch_times(job, jobs, reps, rounds)
        out[f"batch_{jobs}_jobs"] = {"batched_ms": round(b, 5), "singles_ms": round(s, 5), "singles_over_batched": round(s / b, 3),
                                     "same_elements": same, "gated_valid_blocks_of_a_job": blocks}
    return out


def main():
    ap = fb.parser(single.CASES, ("whole",), iters=5, warmup=1)
    ap.add_argument("--reps", type=int, default=50, help="back-to-back calls per launch timing")
    ap.add_argument("--rounds", type=int, default=7, help="alternating launch timings, of which the median is taken")
    ap.add_argument("--no-occluded", action="store_true", help="skip the occluded sub-pixel clip's IoU")
    a = ap.parse_args()
    dev = fb.device()
    import torch
    from lanpaint_amd import propagate_keys_anchored_visible as pkav
    results = []
    for case in ((a.case,) if a.case else tuple(single.CASES)):
        job = single.make_job(case, dev)
        F = job["shape"][0]
        if a.job:
            masks = keyed.painted(job, [0, F - 1])
            fb.untimed(lambda: pkav.propagate_keys_anchored_visible(job["images"], masks, [0, F - 1], LEVELS, SEARCH, SMOOTH, ANCHOR, OCCLUSION),
                       a.warmup + a.iters)
        else:
            results.append(measure(job, a.iters, a.warmup, a.reps, a.rounds))
            del job
            torch.cuda.empty_cache()
            if not a.no_occluded:
                results[-1]["occluded_subpixel_clip"] = occluded(case, dev)
        torch.cuda.empty_cache()
    if not a.job:
        fb.emit("mask_propagate_keys_anchored_visible", a, results)


if __name__ == "__main__":
    main()
