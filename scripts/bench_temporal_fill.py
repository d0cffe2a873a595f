#!/usr/bin/env python3
"""Video temporal fill benchmark (lanpaint_amd.temporal_fill on the HIP device): one JSON line.

The `clip` (81 frames of 1280 x 720 x 3) and `square` (16 frames of 1024 x 1024 x 3) workloads of scripts/bench_propagate.py -- a
textured disc crossing a panning texture -- with the disc's own mask on every frame, grown by 2 pixels, at the default parameters
(levels 4, search 2, smooth 8, reach 0).  Everything is already on the device.

    whole      temporal_fill.temporal_fill against propagate.propagate_masks (key frame 0, the disc's mask) on the same clip in
               the same process, alternately: featurebench.wall, the median of `iters` runs and their min..max, and the
               ratio.  featurebench.events around the call as well.
    split      between two device events: the copy of the clip and the outputs' allocation; the two pyramids of all frames; the
               fields of all 2 (F - 1) steps; the carries are what is left of the whole call.
    launches   counted by wrapping the modules' launch(): the entry calls by name, next to what the rule says they must be.
    carry      one lp_tfill_carry launch (the middle frame's forward step, `reps` calls back to back between two events) against
               a torch.clone of the bytes it must move: the frame's known bytes and, per masked pixel, the donor's known byte and
               state, the new state, the taps, the sample, source and remaining.
    torch      the same rule in torch operators on the same device, compared element by element with the module's result, on
               `--torch-frames` full-size frames of the case.
    filled     the share of masked pixels of the clip that some frame showed.

    python scripts/bench_temporal_fill.py [--iters 5] [--warmup 1] [--case clip] [--torch-frames 4]
    python scripts/bench_temporal_fill.py --job whole --case clip --iters 3        # the body of a kernel-trace run
"""
from __future__ import annotations

import featurebench as fb

import bench_propagate as single  # the workloads, the field in torch

LEVELS, SEARCH, SMOOTH, REACH, GROW = single.LEVELS, single.SEARCH, single.SMOOTH, 0, 2


def make_job(case, dev, frames=None):
    """bench_propagate's clip with the disc's mask of every frame, grown by GROW pixels: `masks` fp32 [F, H, W]."""
    import torch
    job = single.make_job(case, dev, frames)
    F, H, W = job["shape"]
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    r, cy0, cx0 = min(H, W) / 5 + GROW, H / 3, W / 4
    job["masks"] = torch.stack([((yy - cy0 - 1.5 * t) ** 2 + (xx - cx0 - 4.0 * t) ** 2 <= r * r).float() for t in range(F)])
    return job


# ---- the same rule in torch operators ----------------------------------------------------------------------------------------------------
def _pixel_vectors(vec, H, W):
    import torch
    gh, gw = vec.shape[:2]

    def axis(n, g):
        u = 2 * torch.arange(n, device=vec.device) - 7
        b0 = u >> 4
        return b0.clamp(0, g - 1), (b0 + 1).clamp(0, g - 1), u - 16 * b0
    y0, y1, fy = axis(H, gh)
    x0, x1, fx = axis(W, gw)
    fy, fx = fy[:, None, None], fx[None, :, None]
    top = (16 - fx) * vec[y0][:, x0] + fx * vec[y0][:, x1]
    bot = (16 - fx) * vec[y1][:, x0] + fx * vec[y1][:, x1]
    return ((16 - fy) * top + fy * bot + 128) >> 8


def _sample(images, f, P):
    import torch
    H, W = images.shape[1:3]
    Py, Px = P[:, 0].clamp(0, 16 * (H - 1)), P[:, 1].clamp(0, 16 * (W - 1))
    iy, ix, fy, fx = Py >> 4, Px >> 4, (Py & 15)[:, None], (Px & 15)[:, None]
    iy1, ix1 = (iy + 1).clamp(max=H - 1), (ix + 1).clamp(max=W - 1)

    def mix(a, b, w):                                                  # every product and sum a kernel of its own: nothing fuses
        return torch.where(w == 0, 16.0 * a, (16 - w).float() * a + w.float() * b)
    top, bot = mix(images[f, iy, ix], images[f, iy, ix1], fx), mix(images[f, iy1, ix], images[f, iy1, ix1], fx)
    return mix(top, bot, fy) * (1.0 / 256.0)


def torch_temporal_fill(images, mask, levels=LEVELS, search=SEARCH, smooth=SMOOTH, reach=REACH):
    """temporal_fill in torch operators: (filled, remaining, source)."""
    import torch
    F, H, W = images.shape[:3]
    dev = images.device
    known = ~(mask >= 0.5)
    Y = single.torch_luma(images)
    pyr = [single._pyr(Y[f], levels, True) for f in range(F)]
    kpyr = [single._pyr(known[f].long(), levels, False) for f in range(F)]
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    own = torch.stack([16 * yy, 16 * xx], dim=-1)
    frames = torch.arange(F, device=dev)[:, None, None]
    source = torch.where(known, frames, -1)
    filled = images.clone()
    limit = reach if reach else 1 << 30
    for d in (1, -1):
        order = list(range(F)) if d == 1 else list(range(F - 1, -1, -1))
        org = pos = None
        for donor, t in zip(order, order[1:]):
            vec = None
            for lv in range(levels - 1, -1, -1):
                vec = single.torch_fill_median(*single.torch_match(pyr[t][lv], pyr[donor][lv], kpyr[t][lv], vec, search, smooth, lv == 0))
            s_org = torch.where(known[donor], donor, -1 if org is None else org)
            s_pos = own if pos is None else torch.where(known[donor][..., None], own, pos)
            q = own + _pixel_vectors(vec, H, W)
            inside = (q[..., 0] >= 0) & (q[..., 0] <= 16 * (H - 1)) & (q[..., 1] >= 0) & (q[..., 1] <= 16 * (W - 1))
            i = (q + 8) >> 4
            iy, ix = i[..., 0].clamp(0, H - 1), i[..., 1].clamp(0, W - 1)
            f = s_org[iy, ix]
            found = inside & (f >= 0) & ((t - f).abs() <= limit)
            org = torch.where(known[t], t, torch.where(found, f, -1))
            pos = torch.where(known[t][..., None], own, s_pos[iy, ix] + q - 16 * i)
            write = ~known[t] & (org >= 0)
            if d == -1:
                write &= (source[t] == -1) | ((t - org).abs() < (t - source[t]).abs())
            filled[t][write] = _sample(images, org[write], pos[write])
            source[t][write] = org[write]
    return filled, (~known & (source == -1)).float(), source.int()


# ---- measurements ---------------------------------------------------------------------------------------------------------------------------
def expected_launches(F, levels):
    """What the rule says a call in one chunk is made of."""
    groups = -(-(F - 1) // 32)
    return {"lp_prop_luma": 1, "lp_tfill_known": 1, "lp_prop_match_batch": 2 * levels * groups, "lp_prop_fill_batch": 2 * levels * groups,
            "lp_tfill_carry": 2 * (F - 1)}


def carry_alone(job, reps):
    """One carry launch on the middle frame's forward step, and a clone of the bytes it must move: (ms, ms, bytes)."""
    import torch
    from lanpaint_amd import propagate, temporal_fill as tf
    F, H, W = job["shape"]
    images, t = job["images"], F // 2
    C = images.shape[3]
    luma = propagate.luma_pyramids(images[t - 1:t + 1], LEVELS)
    known = tf.known_pyramids(job["masks"][t - 1:t + 1], 2, LEVELS)
    vec = tf.step_fields(luma, known, [(1, 0)], H, W, LEVELS, SEARCH, SMOOTH)[0]
    bits = [propagate.level_view(known, H, W, 0)[i] for i in (0, 1)]
    filled = images.clone()
    source = torch.full((F, H, W), -1, dtype=torch.int32, device=images.device)
    remaining = torch.zeros((F, H, W), device=images.device)
    state, out = tf.new_state(H, W, images.device), tf.new_state(H, W, images.device)
    state[0].fill_(t - 1)
    state[1].copy_(torch.stack(torch.meshgrid(16 * torch.arange(H, device=images.device), 16 * torch.arange(W, device=images.device),
                                              indexing="ij"), dim=-1))
    run = lambda: tf.carry(vec, bits[1], bits[0], state, images, filled, source, remaining, t, t - 1, 0, False, out)    # noqa: E731
    run()
    ms = fb.events(run, reps)
    masked = int((bits[1] == 0).sum())
    moved = H * W + masked * (1 + 12 + 12 + 4 * C * 4 + C * 4 + 4 + 4)
    blob = torch.empty(moved, dtype=torch.uint8, device=images.device)
    blob.clone()
    return ms, fb.events(blob.clone, reps), moved, masked


def measure(job, iters, warmup, torch_frames, reps):
    import torch
    from lanpaint_amd import propagate, temporal_fill as tf
    F, H, W = job["shape"]
    images, masks = job["images"], job["masks"]
    new = lambda: tf.temporal_fill(images, masks, LEVELS, SEARCH, SMOOTH, REACH)                        # noqa: E731
    old = lambda: propagate.propagate_masks(images, job["mask"], 0, LEVELS, SEARCH, SMOOTH)           # noqa: E731
    names = fb.count_launches(new, propagate, tf)
    got = new()
    again = fb.differing(new(), got)
    masked = int((masks >= 0.5).sum())
    left = int(got[1].sum())
    outside = int(((got[0] != images) & (masks < 0.5)[..., None]).sum())
    ages = (got[2] - torch.arange(F, device=images.device)[:, None, None]).abs()[(masks >= 0.5) & (got[2] >= 0)]
    mean_age, max_age = float(ages.float().mean()), int(ages.max())
    del got, ages
    n = min(torch_frames, F)
    eager = torch_temporal_fill(images[:n], masks[:n])
    from_torch = fb.differing(eager, tf.temporal_fill(images[:n], masks[:n], LEVELS, SEARCH, SMOOTH, REACH))
    del eager
    steps = [(t, t - 1) for t in range(1, F)] + [(t, t + 1) for t in range(F - 2, -1, -1)]
    both = lambda: (propagate.luma_pyramids(images, LEVELS), tf.known_pyramids(masks, F, LEVELS))    # noqa: E731
    luma, known = both()
    fields = lambda: [tf.step_fields(luma, known, part, H, W, LEVELS, SEARCH, SMOOTH) for part in (steps[:F - 1], steps[F - 1:])]    # noqa: E731
    copies = lambda: (images.clone(), torch.empty((F, H, W), dtype=torch.int32, device=images.device),    # noqa: E731
                      torch.empty((F, H, W), device=images.device))
    fb.untimed(lambda: (new(), old(), fields()), warmup)
    s = fb.series([("new", new, fb.wall), ("old", old, fb.wall),      # alternating: the two share whatever else the host does
                   ("events", new), ("pyramids", both), ("fields", fields), ("copies", copies),
                   ("torch", lambda: torch_temporal_fill(images[:n], masks[:n]), fb.wall),
                   ("small", lambda: tf.temporal_fill(images[:n], masks[:n], LEVELS, SEARCH, SMOOTH, REACH), fb.wall)], iters, 0)
    new_ms, old_ms, evs, pyr_ms, field_ms, copy_ms, torch_ms, small_ms = s.values()
    del luma, known
    carry_ms, clone_ms, moved, carry_masked = carry_alone(job, reps)
    med = fb.median
    per = {k: names.count(k) for k in sorted(set(names))}
    rest = med(evs) - med(pyr_ms) - med(field_ms) - med(copy_ms)
    return {"case": job["case"], "frames_height_width": [F, H, W], "levels": LEVELS, "search": SEARCH, "smooth": SMOOTH, "reach": REACH,
            "fill_wall_ms": round(med(new_ms), 3), "fill_wall_min_max_ms": fb.summary(new_ms, 3)[1],
            "fill_events_ms": round(med(evs), 3), "ms_per_frame": round(med(new_ms) / F, 4),
            "propagate_wall_ms": round(med(old_ms), 3), "propagate_wall_min_max_ms": fb.summary(old_ms, 3)[1],
            "fill_over_propagate": round(med(new_ms) / med(old_ms), 3),
            "split_ms": {"copy_and_outputs": round(med(copy_ms), 3), "pyramids": round(med(pyr_ms), 3), "fields": round(med(field_ms), 3),
                         "carries_by_difference": round(rest, 3)},
            "carry_ms_per_step_by_difference": round(rest / (2 * (F - 1)), 5),
            "entry_calls": len(names), "entry_calls_by_name": per, "entry_calls_by_the_rule": expected_launches(F, LEVELS),
            "carry_alone_ms": round(carry_ms, 5), "clone_of_its_bytes_ms": round(clone_ms, 5), "carry_bytes": moved,
            "carry_masked_pixels": carry_masked, "carry_over_clone": round(carry_ms / clone_ms, 2), "stage_reps": reps,
            "masked_pixels": masked, "remaining_pixels": left, "share_filled": round(1 - left / max(masked, 1), 4),
            "mean_age_frames": round(mean_age, 2), "max_age_frames": max_age, "elements_changed_outside_the_mask": outside,
            "elements_differing_between_two_calls": again,
            "torch_frames": n, "torch_ms": round(med(torch_ms), 3), "module_ms_same_frames": round(med(small_ms), 3),
            "torch_over_module": round(med(torch_ms) / med(small_ms), 2), "elements_differing_from_torch": from_torch}


def main():
    ap = fb.parser(single.CASES, ("whole",), iters=5, warmup=1)
    ap.add_argument("--reps", type=int, default=50, help="back-to-back calls per stage timing")
    ap.add_argument("--torch-frames", type=int, default=4)
    a = ap.parse_args()
    dev = fb.device()
    import torch
    from lanpaint_amd import temporal_fill as tf
    results = []
    for case in ((a.case,) if a.case else tuple(single.CASES)):
        job = make_job(case, dev)
        if a.job:
            fb.untimed(lambda: tf.temporal_fill(job["images"], job["masks"], LEVELS, SEARCH, SMOOTH, REACH), a.warmup + a.iters)
        else:
            results.append(measure(job, a.iters, a.warmup, a.torch_frames, a.reps))
        del job
        torch.cuda.empty_cache()
    if not a.job:
        fb.emit("video_temporal_fill", a, results)


if __name__ == "__main__":
    main()
