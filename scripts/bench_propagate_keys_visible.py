#!/usr/bin/env python3
"""Occlusion-aware video mask propagate from several keyframes (lanpaint_amd.propagate_keys_visible on the HIP device): one JSON line.

The `clip` (81 frames of 1280 x 720 x 3) and `square` (16 frames of 1024 x 1024 x 3) workloads of scripts/bench_propagate.py with
the bar of scripts/bench_propagate_visible.py drawn over them, at the default parameters, the true disc painted on every key, with
keys on both ends and with a third key in the middle.  Everything is already on the device.

    whole      propagate_keys_visible.propagate_keys_visible against propagate_keys.propagate_keys (the several-keys rule without
               occlusion handling) on the same clip and keys in the same process, alternately: featurebench.wall, the median
               of `iters` runs and their min..max, and the ratio.
    launches   counted by wrapping the modules' launch(): the entry calls by name and the dependent steps.
    stages     the three new entries alone, featurebench.events, `reps` calls back to back: lp_prop_visible_batch and
               lp_prop_occlude_batch with as many jobs as the call's first step has chains, on the call's own first-step buffers,
               and lp_prop_merge_visible on the first gap.  The two EDTs of the gaps alone, and their share of the call.
    checks     two calls give the same bits; the keys return their paintings; the mask pixels on the bar against the plain rule's.

    python scripts/bench_propagate_keys_visible.py [--iters 5] [--warmup 1] [--case clip] [--keys ends]
    python scripts/bench_propagate_keys_visible.py --job whole --case clip --keys ends     # the body of a kernel-trace run
"""
from __future__ import annotations

import featurebench as fb

import bench_propagate as single  # the cases and parameters
import bench_propagate_keys as several  # the paintings
import bench_propagate_visible as visible  # the clip with the bar

LEVELS, SEARCH, SMOOTH, OCCLUSION = single.LEVELS, single.SEARCH, single.SMOOTH, visible.OCCLUSION
KEY_SETS = {"ends": lambda F: [0, F - 1], "ends and middle": lambda F: [0, F // 2, F - 1]}


def stage_times(job, masks, keys, reps):
    """The three new entries alone, ms per call: the two batch entries with the first step's jobs on buffers of their own, the
    merge on the first gap's frames."""
    import numpy as np
    import torch
    from lanpaint_amd import _cabi, propagate, propagate_keys, propagate_keys_visible as kv, stabilize
    F, H, W = job["shape"]
    dev = job["images"].device
    plan = propagate_keys.chain_plan(F, keys)
    jobs = min(len(plan), kv.MAX_JOBS)
    pyr = propagate_keys.clip_pyramids(job["images"][:2], LEVELS)
    mpyr, bits = propagate.key_mask(masks[0], LEVELS)
    luma = [propagate.level_view(pyr[i:i + 1], H, W, 0)[0] for i in (0, 1)]
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    pos = torch.stack([16 * yy, 16 * xx], dim=-1).int().contiguous()
    key_bits = propagate.level_view(mpyr, H, W, 0)[0]
    out = {"jobs": jobs}
    feed = [(pos, luma[1], luma[0], key_bits)] * jobs
    out["visible_batch"] = fb.events(lambda: kv.visible_flags_batch(feed, OCCLUSION), reps)
    flags = kv.visible_flags_batch(feed[:1], OCCLUSION)[0]
    counts = torch.zeros(jobs, dtype=torch.int32, device=dev)
    out["occlude_batch"] = fb.events(lambda: kv.occlude_batch([(bits, flags)] * jobs, LEVELS, counts), reps)
    a, b = next((a, b) for a, b in zip(keys, keys[1:]) if b - a > 1)
    n, span = b - a - 1, b - a
    code = bits[None].repeat(n, 1, 1)
    q = stabilize.signed_d2(code)
    fl = torch.zeros((n, *_cabi.prop_grid(H, W)), dtype=torch.int32, device=dev)
    many = torch.from_numpy(np.full(span, 1000, np.int32)).to(dev)
    o, h = torch.empty_like(code), torch.empty_like(code)
    out["merge_visible"] = fb.events(lambda: kv.merge_gap_visible(q, q, code, code, code, code, fl, fl, many, many, span, 1, o, h), reps)
    out["merge_visible_frames"] = n
    lost = many.clone()
    lost[1] = 0                                                       # the forward chain lost on every frame: the pass-through branch
    out["merge_visible_one_lost"] = fb.events(lambda: kv.merge_gap_visible(q, q, code, code, code, code, fl, fl, lost, many, span, 1, o, h), reps)
    torch.cuda.synchronize()
    return out


def measure(job, name, keys, iters, warmup, reps):
    from lanpaint_amd import propagate_keys, propagate_keys_visible as kv, stabilize
    F, H, W = job["shape"]
    masks = several.painted(job, keys)
    new = lambda: kv.propagate_keys_visible(job["images"], masks, keys, LEVELS, SEARCH, SMOOTH, OCCLUSION)    # noqa: E731
    old = lambda: propagate_keys.propagate_keys(job["images"], masks, keys, LEVELS, SEARCH, SMOOTH)          # noqa: E731
    names = fb.count_launches(new, propagate_keys, kv)
    got, hid = new()
    differing_again = fb.differing(new(), (got, hid))
    plain = old()
    x0, x1 = job["bar"]
    on_bar, on_bar_plain = int((got[:, :, x0:x1] >= 0.5).sum()), int((plain[:, :, x0:x1] >= 0.5).sum())
    keys_differing = int(sum(((got[k] != (masks[i] >= 0.5).float()).sum() + (hid[k] != 0).sum()) for i, k in enumerate(keys)))
    truth = several.painted(job, list(range(F))) >= 0.5
    subject = (got + hid) >= 0.5
    inter = (subject & truth).flatten(1).sum(1).double()
    union = (subject | truth).flatten(1).sum(1).clamp(min=1).double()
    iou = float((inter / union).min())
    hidden_mass = float(hid.sum())
    del truth, subject, plain
    gaps = [(a, b) for a, b in zip(keys, keys[1:]) if b - a > 1]
    edt_of = lambda: [stabilize.signed_d2(got[a + 1:b]) for a, b in gaps for _ in range(2)]    # noqa: E731
    # alternating: the two share whatever else the host does
    fb.untimed(lambda: (new(), old()), warmup)
    new_ms, old_ms, edts = fb.series([("new", new, fb.wall), ("old", old, fb.wall), ("edt", edt_of)], iters, 0).values()
    stages = stage_times(job, masks, keys, reps)
    med = fb.median
    plan = propagate_keys.chain_plan(F, keys)
    steps = max((c[3] for c in plan), default=0)
    return {"case": job["case"], "keys": name, "key_frames": keys, "frames_height_width": [F, H, W], "levels": LEVELS, "occlusion": OCCLUSION,
            "visible_wall_ms": round(med(new_ms), 3), "visible_wall_min_max_ms": fb.summary(new_ms, 3)[1],
            "keys_wall_ms": round(med(old_ms), 3), "keys_wall_min_max_ms": fb.summary(old_ms, 3)[1],
            "visible_over_keys": round(med(new_ms) / med(old_ms), 3),
            "chains": len(plan), "dependent_steps": steps, "entry_calls": len(names),
            "entry_calls_by_name": {k: names.count(k) for k in sorted(set(names))},
            "stage_ms": {k: (round(v, 5) if isinstance(v, float) else v) for k, v in stages.items()}, "stage_reps": reps,
            "new_step_launches_ms_per_call": round(steps * (stages["visible_batch"] + stages["occlude_batch"]), 4),
            "edt_ms": round(med(edts), 3), "edt_share": round(med(edts) / med(new_ms), 3),
            "mask_pixels_on_bar": on_bar, "mask_pixels_on_bar_keys": on_bar_plain, "hidden_mass": round(hidden_mass, 1),
            "subject_iou_minimum_over_frames": round(iou, 4), "elements_differing_on_the_keys": keys_differing,
            "elements_differing_between_two_calls": differing_again}


def main():
    ap = fb.parser(single.CASES, ("whole",), iters=5, warmup=1)
    ap.add_argument("--reps", type=int, default=20, help="back-to-back calls per stage timing")
    ap.add_argument("--keys", choices=tuple(KEY_SETS), help="this set of keys only")
    a = ap.parse_args()
    dev = fb.device()
    import torch
    from lanpaint_amd import propagate_keys_visible as kv
    results = []
    for case in ((a.case,) if a.case else tuple(single.CASES)):
        job = visible.make_job(case, dev)
        F = job["shape"][0]
        for name in ((a.keys,) if a.keys else tuple(KEY_SETS)):
            keys = KEY_SETS[name](F)
            if a.job:
                masks = several.painted(job, keys)
                fb.untimed(lambda: kv.propagate_keys_visible(job["images"], masks, keys, LEVELS, SEARCH, SMOOTH, OCCLUSION), a.warmup + a.iters)
            else:
                results.append(measure(job, name, keys, a.iters, a.warmup, a.reps))
                torch.cuda.empty_cache()
        del job
        torch.cuda.empty_cache()
    if not a.job:
        fb.emit("mask_propagate_keys_visible", a, results)


if __name__ == "__main__":
    main()
