#!/usr/bin/env python3
"""Video temporal smooth benchmark (lanpaint_amd.temporal_smooth on the HIP device): one JSON line.

The `clip` (81 frames of 1280 x 720 x 3) and `square` (16 frames of 1024 x 1024 x 3) workloads of scripts/bench_temporal_fill.py -- a
textured disc crossing a panning texture, the disc's own mask on every frame, grown by 2 pixels -- at the default parameters
(tolerance 24, motion "background", levels 4, search 2, smooth 8) and at radius 1, 2 (the default) and 8.  Everything is already on
the device.

    whole      temporal_smooth.temporal_smooth per radius against temporal_fill.temporal_fill on the same clip in the same process,
               alternately: featurebench.wall, the median of `iters` runs and their min..max, and the ratio.
               featurebench.events around the call as well.
    split      between two device events, per radius: the two pyramids of all frames, the fields of all 2 (F - 1) steps, and the one
               smooth launch for all frames (`reps` calls back to back).
    launch     that launch against a clone of a buffer of the bytes it must move: every frame read and written once, the known
               bytes, support, and per masked pixel and step the four block vectors and the taps (all 2 R steps, as if none
               ended).  The same launch with an empty mask -- the copy alone -- against a clone of the clip.  A clone here is
               what torch.clone runs, `copy_` into a buffer allocated beforehand: a fresh allocation of gigabytes inside the
               timed window measured the allocator (1.6 ms one run, 28 ms the next).
    launches   counted by wrapping the modules' launch(): the entry calls by name.
    torch      the same rule in torch operators on the same device, compared element by element with the module's result, on
               `--torch-frames` full-size frames of the case.
    support    the mean of support / (2 R) under the mask, and the elements changed outside it.

    python scripts/bench_temporal_smooth.py [--iters 5] [--warmup 1] [--case clip] [--torch-frames 4]
    python scripts/bench_temporal_smooth.py --job whole --case clip --iters 3       # the body of a kernel-trace run
"""
from __future__ import annotations

from math import comb

import featurebench as fb

import bench_propagate as single  # the field in torch
import bench_temporal_fill as fill  # the workloads, the vectors and the sample in torch

LEVELS, SEARCH, SMOOTH, TOLERANCE, MOTION, RADII = single.LEVELS, single.SEARCH, single.SMOOTH, 24, "background", (1, 2, 8)


# ---- the same rule in torch operators ----------------------------------------------------------------------------------------------------
def _codes(v):
    import torch
    t = torch.where(v > 0, v.clamp(max=1.0), torch.zeros_like(v))     # a NaN gives 0
    return (t * 255.0 + 0.5).int()                                     # the product and the sum are kernels of their own


def torch_temporal_smooth(images, mask, radius, tolerance=TOLERANCE, motion=MOTION, levels=LEVELS, search=SEARCH, smooth=SMOOTH):
    """temporal_smooth in torch operators: (out, support)."""
    import torch
    F, H, W = images.shape[:3]
    known = ~(mask >= 0.5)
    Y = single.torch_luma(images)
    pyr = [single._pyr(Y[f], levels, True) for f in range(F)]
    kpyr = [single._pyr((known[f] if motion == "background" else torch.ones_like(known[f])).long(), levels, False) for f in range(F)]
    V = {}

    def vectors(u, v):
        if (u, v) not in V:
            vec = None
            for lv in range(levels - 1, -1, -1):
                vec = single.torch_fill_median(*single.torch_match(pyr[u][lv], pyr[v][lv], kpyr[u][lv], vec, search, smooth, lv == 0))
            V[(u, v)] = fill._pixel_vectors(vec, H, W)
        return V[(u, v)]
    w = [comb(2 * radius, radius + k) for k in range(radius + 1)]
    out = images.clone()
    support = torch.full((F, H, W), -1, dtype=torch.int32, device=images.device)
    for t in range(F):
        ys, xs = torch.nonzero(~known[t], as_tuple=True)
        x = images[t, ys, xs]
        cx = _codes(x)
        acc = torch.zeros_like(x)
        total = torch.full_like(ys, w[0])
        count = torch.zeros_like(ys)
        for d in (-1, 1):
            alive = torch.ones_like(ys, dtype=torch.bool)
            p = torch.stack([16 * ys, 16 * xs], dim=-1)
            for k in range(1, radius + 1):
                u, v = t + (k - 1) * d, t + k * d
                if v < 0 or v >= F:
                    break
                i = (p + 8) >> 4
                q = p + vectors(u, v)[i[:, 0].clamp(0, H - 1), i[:, 1].clamp(0, W - 1)]
                alive = alive & (q[:, 0] >= 0) & (q[:, 0] <= 16 * (H - 1)) & (q[:, 1] >= 0) & (q[:, 1] <= 16 * (W - 1))
                s = fill._sample(images, torch.full_like(ys, v), q)
                alive = alive & ((_codes(s) - cx).abs().amax(dim=1) <= tolerance)
                term = float(w[k]) * (s - x)
                acc = torch.where(alive[:, None], acc + term, acc)
                total = total + torch.where(alive, w[k], 0)
                count = count + alive
                p = torch.where(alive[:, None], q, p)
        new = x + acc / total.float()[:, None]
        out[t, ys, xs] = torch.where((count > 0)[:, None], new, x)
        support[t, ys, xs] = count.int()
    return out, support


# ---- measurements ---------------------------------------------------------------------------------------------------------------------------
def measure(job, iters, warmup, torch_frames, reps):
    import torch
    from lanpaint_amd import propagate, temporal_fill as tf, temporal_smooth as ts
    F, H, W = job["shape"]
    images, masks = job["images"], job["masks"]
    C = images.shape[3]
    old = lambda: tf.temporal_fill(images, masks, LEVELS, SEARCH, SMOOTH, 0)                            # noqa: E731
    med = fb.median
    masked = int((masks >= 0.5).sum())
    n = min(torch_frames, F)
    both = lambda: (propagate.luma_pyramids(images, LEVELS), tf.known_pyramids(masks, F, LEVELS))    # noqa: E731
    luma, known = both()
    per_radius = []
    for radius in RADII:
        new = lambda: ts.temporal_smooth(images, masks, radius, TOLERANCE, MOTION, LEVELS, SEARCH, SMOOTH)    # noqa: E731
        names = fb.count_launches(new, propagate, tf, ts)
        got = new()
        again = fb.differing(new(), got)
        outside = int(((got[0] != images) & (masks < 0.5)[..., None]).sum())
        changed = int(((got[0] != images).any(dim=-1) & (masks >= 0.5)).sum())
        share = float(got[1][masks >= 0.5].float().mean()) / (2 * radius)
        del got
        eager = torch_temporal_smooth(images[:n], masks[:n], radius)
        from_torch = fb.differing(eager, ts.temporal_smooth(images[:n], masks[:n], radius, TOLERANCE, MOTION, LEVELS, SEARCH, SMOOTH))
        del eager
        fwd, bwd = ts.field_steps(0, F, F, radius)
        steps = [(u, u + 1) for u in fwd] + [(u, u - 1) for u in bwd]
        fields = lambda: tf.step_fields(luma, known, steps, H, W, LEVELS, SEARCH, SMOOTH)               # noqa: E731
        vec = fields()
        out = torch.empty_like(images)
        support = torch.empty((F, H, W), dtype=torch.int32, device=images.device)
        alone = lambda: ts.smooth_frames(vec[:len(fwd)], vec[len(fwd):], known, images, radius, TOLERANCE, 0, F, 0, 1, out, support)    # noqa: E731
        fb.untimed(lambda: (new(), old(), fields(), alone()), warmup)
        s = fb.series([("new", new, fb.wall), ("old", old, fb.wall),  # alternating: the two share whatever else the host does
                       ("events", new), ("pyramids", both), ("fields", fields),
                       ("torch", lambda: torch_temporal_smooth(images[:n], masks[:n], radius), fb.wall),
                       ("small", lambda: ts.temporal_smooth(images[:n], masks[:n], radius, TOLERANCE, MOTION, LEVELS, SEARCH, SMOOTH), fb.wall)],
                      iters, 0)
        new_ms, old_ms, evs, pyr_ms, field_ms, torch_ms, small_ms = s.values()
        launch_ms = fb.events(alone, reps)
        all_known = torch.ones((F, H, W), dtype=torch.uint8, device=images.device)
        copy_only = lambda: ts.smooth_frames(vec[:len(fwd)], vec[len(fwd):], all_known, images, radius, TOLERANCE, 0, F, 0, 1, out, support)    # noqa: E731
        copy_only()
        copy_ms = fb.events(copy_only, reps)
        frames_clone_ms = fb.events(lambda: out.copy_(images), reps)        # what torch.clone runs, without its allocation
        del all_known
        moved = F * H * W * (2 * C * 4 + 1 + 4) + masked * 2 * radius * (4 * 8 + 4 * C * 4)
        blob, twin = (torch.empty(moved, dtype=torch.uint8, device=images.device) for _ in range(2))
        twin.copy_(blob)
        clone_ms = fb.events(lambda: twin.copy_(blob), max(reps // 5, 1))
        del blob, twin, vec, out, support
        per_radius.append({
            "radius": radius, "smooth_wall_ms": round(med(new_ms), 3), "smooth_wall_min_max_ms": fb.summary(new_ms, 3)[1],
            "smooth_events_ms": round(med(evs), 3), "ms_per_frame": round(med(new_ms) / F, 4),
            "fill_wall_ms": round(med(old_ms), 3), "fill_wall_min_max_ms": fb.summary(old_ms, 3)[1],
            "smooth_over_fill": round(med(new_ms) / med(old_ms), 3),
            "split_ms": {"pyramids": round(med(pyr_ms), 3), "fields": round(med(field_ms), 3), "smooth_launch": round(launch_ms, 4),
                         "smooth_launch_with_an_empty_mask": round(copy_ms, 4), "clone_of_the_clip": round(frames_clone_ms, 4)},
            "fields_share": round(med(field_ms) / med(evs), 3),
            "launch_bytes": moved, "clone_of_its_bytes_ms": round(clone_ms, 4), "launch_over_clone": round(launch_ms / clone_ms, 2),
            "entry_calls": len(names), "entry_calls_by_name": {k: names.count(k) for k in sorted(set(names))},
            "mean_support_share": round(share, 4), "masked_pixels_changed": changed, "elements_changed_outside_the_mask": outside,
            "elements_differing_between_two_calls": again,
            "torch_frames": n, "torch_ms": round(med(torch_ms), 3), "module_ms_same_frames": round(med(small_ms), 3),
            "torch_over_module": round(med(torch_ms) / med(small_ms), 2), "elements_differing_from_torch": from_torch})
    return {"case": job["case"], "frames_height_width": [F, H, W], "tolerance": TOLERANCE, "motion": MOTION, "levels": LEVELS,
            "search": SEARCH, "smooth": SMOOTH, "masked_pixels": masked, "stage_reps": reps, "radii": per_radius}


def main():
    ap = fb.parser(single.CASES, ("whole",), iters=5, warmup=1)
    ap.add_argument("--reps", type=int, default=50, help="back-to-back calls per stage timing")
    ap.add_argument("--torch-frames", type=int, default=4)
    a = ap.parse_args()
    dev = fb.device()
    import torch
    from lanpaint_amd import temporal_smooth as ts
    results = []
    for case in ((a.case,) if a.case else tuple(single.CASES)):
        job = fill.make_job(case, dev)
        if a.job:
            fb.untimed(lambda: ts.temporal_smooth(job["images"], job["masks"], 2, TOLERANCE, MOTION, LEVELS, SEARCH, SMOOTH), a.warmup + a.iters)
        else:
            results.append(measure(job, a.iters, a.warmup, a.torch_frames, a.reps))
        del job
        torch.cuda.empty_cache()
    if not a.job:
        fb.emit("video_temporal_smooth", a, results)


if __name__ == "__main__":
    main()
