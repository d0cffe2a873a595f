#!/usr/bin/env python3
"""Video mask propagate from several keyframes (lanpaint_amd.propagate_keys on the HIP device): one JSON line.

The `clip` (81 frames of 1280 x 720 x 3) and `square` (16 frames of 1024 x 1024 x 3) workloads of scripts/bench_propagate.py at
the default parameters, the true disc painted on every key, with three sets of keys: the two ends, the two ends and the middle,
every 10th frame.  Everything is already on the device.

    whole      propagate_keys.propagate_keys, featurebench.wall: the median of `iters` runs and their min..max.
    launches   counted by wrapping the module's launch(): the batched entry calls, the merges, and the dependent steps (the
               longest chain).
    edt        stabilize.signed_d2 on every gap's two stacks alone, featurebench.events, and its share of the whole call.
    composed   the same result from what the single-key module already has: one propagate.propagate_masks per key on the frames
               between its neighbouring keys, stabilize.signed_d2 on the two results of a gap, and the merge in torch fp64
               operators, on the same device.  Timed the same way and compared element by element.  This is the yardstick: the
               batched call must not be slower than it.

    python scripts/bench_propagate_keys.py [--iters 5] [--warmup 1] [--case clip]
    python scripts/bench_propagate_keys.py --job whole --case clip --keys ends     # the body of a kernel-trace run
"""
from __future__ import annotations

import featurebench as fb

import bench_propagate as single

LEVELS, SEARCH, SMOOTH = single.LEVELS, single.SEARCH, single.SMOOTH
KEY_SETS = {"ends": lambda F: [0, F - 1], "ends and middle": lambda F: [0, F // 2, F - 1],
            "every 10th": lambda F: sorted(set(range(0, F, 10)) | {F - 1})}


def painted(job, keys):
    """The true disc of scripts/bench_propagate.py's scene on every key frame: fp32 [K, H, W]."""
    import torch
    F, H, W = job["shape"]
    dev = job["images"].device
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    r, cy0, cx0 = min(H, W) / 5, H / 3, W / 4
    return torch.stack([((yy - cy0 - 1.5 * t) ** 2 + (xx - cx0 - 4.0 * t) ** 2 <= r * r).float() for t in keys])


def torch_merge(qa, qb, n):
    """lp_prop_merge in torch fp64 operators, every product and sum an operator of its own: frames 1..n - 1 of a gap."""
    import torch
    def capped(q):
        return torch.sign(q).double() * torch.sqrt(q.abs().clamp(max=4096).double())
    j = torch.arange(1, n, device=qa.device, dtype=torch.float64)[:, None, None]
    pa = (n - j) * capped(qa)
    pb = j * capped(qb)
    acc = pa + pb
    sd = acc / float(n)
    return (0.5 + sd).clamp(0.0, 1.0).float()


def composed(images, masks, keys):
    """The rule from the single-key module's parts: a propagate_masks per key on its span, signed_d2, the merge in torch."""
    import torch
    from lanpaint_amd import propagate, stabilize
    F, H, W = images.shape[:3]
    out = torch.empty((F, H, W), dtype=torch.float32, device=images.device)
    spans = []
    for i, k in enumerate(keys):
        lo = keys[i - 1] + 1 if i else 0
        hi = keys[i + 1] - 1 if i + 1 < len(keys) else F - 1
        spans.append((lo, propagate.propagate_masks(images[lo:hi + 1], masks[i], k - lo, LEVELS, SEARCH, SMOOTH)))
    for i, k in enumerate(keys):
        lo, res = spans[i]
        if i == 0:
            out[:k + 1] = res[:k + 1 - lo]
        if i + 1 == len(keys):
            out[k:] = res[k - lo:]
        else:
            out[k] = res[k - lo]
            b = keys[i + 1]
            if b - k > 1:
                lo_b, res_b = spans[i + 1]
                A, B = res[k + 1 - lo:b - lo], res_b[k + 1 - lo_b:b - lo_b]
                out[k + 1:b] = torch_merge(stabilize.signed_d2(A.contiguous()), stabilize.signed_d2(B.contiguous()), b - k)
    return out


def measure(job, name, keys, iters, warmup):
    from lanpaint_amd import propagate_keys, stabilize
    F, H, W = job["shape"]
    masks = painted(job, keys)
    call = lambda: propagate_keys.propagate_keys(job["images"], masks, keys, LEVELS, SEARCH, SMOOTH)    # noqa: E731
    other = lambda: composed(job["images"], masks, keys)              # noqa: E731
    names = fb.count_launches(call, propagate_keys)
    got = call()
    differing = fb.differing(other(), got)
    again = fb.differing(call(), got)
    truth = painted(job, list(range(F))) >= 0.5
    inter = ((got >= 0.5) & truth).flatten(1).sum(1).double()
    union = ((got >= 0.5) | truth).flatten(1).sum(1).clamp(min=1).double()
    iou = float((inter / union).min())
    del truth
    gaps = [(a, b) for a, b in zip(keys, keys[1:]) if b - a > 1]
    edt_of = lambda: [stabilize.signed_d2(got[a + 1:b]) for a, b in gaps for _ in range(2)]    # noqa: E731
    fb.untimed(lambda: (call(), other()), warmup)
    walls, others, edts = fb.series([("whole", call, fb.wall), ("composed", other, fb.wall), ("edt", edt_of)], iters, 0).values()
    med = fb.median
    plan = propagate_keys.chain_plan(F, keys)
    spread = max(walls) - min(walls)
    return {"case": job["case"], "keys": name, "key_frames": keys, "frames_height_width": [F, H, W],
            "whole_wall_ms": round(med(walls), 3), "whole_wall_min_max_ms": fb.summary(walls, 3)[1],
            "composed_wall_ms": round(med(others), 3), "composed_wall_min_max_ms": fb.summary(others, 3)[1],
            "composed_over_batched": round(med(others) / med(walls), 3),
            "batched_not_slower_beyond_spread": bool(med(walls) <= med(others) + spread),
            "elements_differing_from_composed": differing, "elements_differing_between_two_calls": again,
            "chains": len(plan), "dependent_steps": max((c[3] for c in plan), default=0),
            "dependent_steps_one_after_another": sum(c[3] for c in plan),
            "entry_calls": len(names), "batched_entry_calls": sum(n.endswith("_batch") for n in names),
            "entry_calls_by_name": {k: names.count(k) for k in sorted(set(names))},
            "edt_ms": round(med(edts), 3), "edt_share": round(med(edts) / med(walls), 3), "iou_minimum_over_frames": round(iou, 4)}


def main():
    ap = fb.parser(single.CASES, ("whole",), iters=5, warmup=1)
    ap.add_argument("--keys", choices=tuple(KEY_SETS), help="this set of keys only")
    a = ap.parse_args()
    dev = fb.device()
    import torch
    from lanpaint_amd import propagate_keys
    results = []
    for case in ((a.case,) if a.case else tuple(single.CASES)):
        job = single.make_job(case, dev)
        F = job["shape"][0]
        for name in ((a.keys,) if a.keys else tuple(KEY_SETS)):
            keys = KEY_SETS[name](F)
            if a.job:
                masks = painted(job, keys)
                fb.untimed(lambda: propagate_keys.propagate_keys(job["images"], masks, keys, LEVELS, SEARCH, SMOOTH), a.warmup + a.iters)
            else:
                results.append(measure(job, name, keys, a.iters, a.warmup))
                torch.cuda.empty_cache()
        del job
        torch.cuda.empty_cache()
    if not a.job:
        fb.emit("mask_propagate_keys", a, results)


if __name__ == "__main__":
    main()
