#!/usr/bin/env python3
"""Robust video temporal smooth benchmark (lanpaint_amd.temporal_smooth_robust on the HIP device): one JSON line.

The `clip` (81 frames of 1280 x 720 x 3) and `square` (16 frames of 1024 x 1024 x 3) workloads of scripts/bench_temporal_smooth.py,
at its parameters (tolerance 24, motion "background", levels 4, search 2, smooth 8) and at radius 1, 2 (the default) and 8.
Everything is already on the device.

    whole      temporal_smooth_robust.temporal_smooth_robust per radius against temporal_smooth.temporal_smooth on the same clip in
               the same process, alternately: featurebench.wall, the median of `iters` runs and their min..max, and the
               ratio.  featurebench.events around the robust call as well.
    launch     the one launch alone (`robust_frames`) against the plain one (`smooth_frames`) on the same fields, `reps` calls back
               to back between two device events, and the ratio; both with an empty mask too -- the copy alone.
    resources  VGPRs, SGPRs, LDS and scratch of the two kernels, from the metadata of the library that ran.
    pop        the clip with 64 / 256 added under the mask of the middle frame, with the motion "background" and "picture": the
               error against the clean clip in that frame before, after the robust and after the plain call (mean and largest
               under the mask); beside them what the two calls move on the clean clip itself, the pixels replaced in that frame,
               and those replaced elsewhere.
    checks     two calls differ in 0 elements; 0 elements change outside the mask; the pixels replaced on the clean clip.

    python scripts/bench_temporal_smooth_robust.py [--iters 5] [--warmup 1] [--reps 20] [--case clip]
    python scripts/bench_temporal_smooth_robust.py --job whole --case clip --iters 3       # the body of a kernel-trace run
"""
from __future__ import annotations

import featurebench as fb

import bench_propagate as single  # the cases
import bench_temporal_fill as fill  # the workloads
import bench_temporal_smooth as plain  # the parameters

LEVELS, SEARCH, SMOOTH, TOLERANCE, MOTION, RADII = plain.LEVELS, plain.SEARCH, plain.SMOOTH, plain.TOLERANCE, plain.MOTION, plain.RADII
POP = 64 / 256


def kernel_resources():
    import instantiation_coverage as ic
    from lanpaint_amd import _cabi
    out = {}
    for name, k in ic.kernel_resources(_cabi.LIB_PATH).items():
        for short in ("lp_tsmooth_kernel", "lp_tsmooth_robust_kernel"):
            if short + "E" in name:
                out[short] = {"vgprs": k[".vgpr_count"], "sgprs": k[".sgpr_count"], "lds_bytes": k[".group_segment_fixed_size"],
                              "scratch_bytes": k[".private_segment_fixed_size"], "vgpr_spills": k[".vgpr_spill_count"],
                              "max_lanes_a_block": k[".max_flat_workgroup_size"]}
    return out


def pop_errors(job, radius):
    """The pop in the middle frame, per motion."""
    import torch
    from lanpaint_amd import temporal_smooth as ts, temporal_smooth_robust as tr
    clean, masks = job["images"], job["masks"]
    t = clean.shape[0] // 2
    under = masks[t] >= 0.5
    popped = clean.clone()
    popped[t][under] += POP
    rows = {}

    def error(result):
        e = (result[t] - clean[t]).abs()[under]
        return {"mean": round(float(e.mean()), 5), "largest": round(float(e.max()), 5)}
    for motion in ts.MOTIONS:
        args = (radius, TOLERANCE, motion, LEVELS, SEARCH, SMOOTH)
        robust, kept = tr.temporal_smooth_robust(popped, masks, *args), ts.temporal_smooth(popped, masks, *args)
        rows[motion] = {"before": error(popped), "after_robust": error(robust[0]), "after_plain": error(kept[0]),
                        "robust_on_the_clean_clip": error(tr.temporal_smooth_robust(clean, masks, *args)[0]),
                        "plain_on_the_clean_clip": error(ts.temporal_smooth(clean, masks, *args)[0]),
                        "masked_pixels_in_the_frame": int(under.sum()), "replaced_in_the_frame": int((robust[2][t] == 1).sum()),
                        "replaced_in_the_other_frames": int((robust[2] == 1).sum() - (robust[2][t] == 1).sum())}
        del robust, kept
    del popped
    torch.cuda.empty_cache()
    return {"frame": t, "radius": radius, "added": POP, "motions": rows}


def measure(job, iters, warmup, reps):
    import torch
    from lanpaint_amd import propagate, temporal_fill as tf, temporal_smooth as ts, temporal_smooth_robust as tr
    F, H, W = job["shape"]
    images, masks = job["images"], job["masks"]
    med = fb.median
    masked = int((masks >= 0.5).sum())
    luma, known = propagate.luma_pyramids(images, LEVELS), tf.known_pyramids(masks, F, LEVELS)
    per_radius = []
    for radius in RADII:
        args = (radius, TOLERANCE, MOTION, LEVELS, SEARCH, SMOOTH)
        new = lambda: tr.temporal_smooth_robust(images, masks, *args)                                    # noqa: E731
        old = lambda: ts.temporal_smooth(images, masks, *args)                                           # noqa: E731
        names = fb.count_launches(new, propagate, tf, ts)
        got = new()
        again = fb.differing(new(), got)
        outside = int(((got[0] != images) & (masks < 0.5)[..., None]).sum())
        replaced = int((got[2] == 1).sum())
        share = float(got[1][masks >= 0.5].float().mean()) / (2 * radius)
        from_plain = int(((got[0] != old()[0]).any(dim=-1)).sum())
        del got
        fwd, bwd = ts.field_steps(0, F, F, radius)
        vec = tf.step_fields(luma, known, [(u, u + 1) for u in fwd] + [(u, u - 1) for u in bwd], H, W, LEVELS, SEARCH, SMOOTH)
        out = torch.empty_like(images)
        support, flags = (torch.empty((F, H, W), dtype=torch.int32, device=images.device) for _ in range(2))
        all_known = torch.ones((F, H, W), dtype=torch.uint8, device=images.device)
        launches = {
            "robust": lambda: tr.robust_frames(vec[:len(fwd)], vec[len(fwd):], known, images, radius, TOLERANCE, 0, F, 0, 1, out, support, flags),
            "plain": lambda: ts.smooth_frames(vec[:len(fwd)], vec[len(fwd):], known, images, radius, TOLERANCE, 0, F, 0, 1, out, support),
            "robust_empty_mask": lambda: tr.robust_frames(vec[:len(fwd)], vec[len(fwd):], all_known, images, radius, TOLERANCE, 0, F, 0, 1,
                                                          out, support, flags),
            "plain_empty_mask": lambda: ts.smooth_frames(vec[:len(fwd)], vec[len(fwd):], all_known, images, radius, TOLERANCE, 0, F, 0, 1,
                                                         out, support)}
        fb.untimed(lambda: (new(), old(), [fn() for fn in launches.values()]), warmup)
        # alternating: the two share whatever else the host does
        new_ms, old_ms, evs = fb.series([("new", new, fb.wall), ("old", old, fb.wall), ("events", new)], iters, 0).values()
        launch_ms = {k: fb.events(fn, reps) for k, fn in launches.items()}
        del vec, out, support, flags, all_known
        per_radius.append({
            "radius": radius, "robust_wall_ms": round(med(new_ms), 3), "robust_wall_min_max_ms": fb.summary(new_ms, 3)[1],
            "robust_events_ms": round(med(evs), 3), "ms_per_frame": round(med(new_ms) / F, 4),
            "plain_wall_ms": round(med(old_ms), 3), "plain_wall_min_max_ms": fb.summary(old_ms, 3)[1],
            "robust_over_plain": round(med(new_ms) / med(old_ms), 3),
            "launch_ms": {k: round(v, 4) for k, v in launch_ms.items()},
            "launch_robust_over_plain": round(launch_ms["robust"] / launch_ms["plain"], 3),
            "launch_robust_over_plain_empty_mask": round(launch_ms["robust_empty_mask"] / launch_ms["plain_empty_mask"], 3),
            "entry_calls": len(names), "entry_calls_by_name": {k: names.count(k) for k in sorted(set(names))},
            "mean_support_share": round(share, 4), "pixels_replaced": replaced, "pixels_differing_from_the_plain_call": from_plain,
            "elements_changed_outside_the_mask": outside, "elements_differing_between_two_calls": again})
    del luma, known
    torch.cuda.empty_cache()
    return {"case": job["case"], "frames_height_width": [F, H, W], "tolerance": TOLERANCE, "motion": MOTION, "levels": LEVELS,
            "search": SEARCH, "smooth": SMOOTH, "masked_pixels": masked, "stage_reps": reps, "radii": per_radius,
            "pop": pop_errors(job, 2)}


def main():
    ap = fb.parser(single.CASES, ("whole",), iters=5, warmup=1)
    ap.add_argument("--reps", type=int, default=20, help="back-to-back calls per launch timing")
    a = ap.parse_args()
    dev = fb.device()
    import torch
    from lanpaint_amd import temporal_smooth_robust as tr
    results = []
    for case in ((a.case,) if a.case else tuple(single.CASES)):
        job = fill.make_job(case, dev)
        job.setdefault("case", case)
        if a.job:
            fb.untimed(lambda: tr.temporal_smooth_robust(job["images"], job["masks"], 2, TOLERANCE, MOTION, LEVELS, SEARCH, SMOOTH), a.warmup + a.iters)
        else:
            results.append(measure(job, a.iters, a.warmup, a.reps))
        del job
        torch.cuda.empty_cache()
    if not a.job:
        fb.emit("video_temporal_smooth_robust", a, results, kernels=kernel_resources())


if __name__ == "__main__":
    main()
