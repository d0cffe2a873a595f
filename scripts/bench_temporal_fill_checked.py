#!/usr/bin/env python3
"""Checked video temporal fill benchmark (lanpaint_amd.temporal_fill_checked on the HIP device): one JSON line.

The two workloads of scripts/bench_temporal_fill.py -- `clip` (81 frames of 1280 x 720 x 3) and `square` (16 frames of
1024 x 1024 x 3), a textured disc crossing a panning texture under its own mask grown by 2 pixels -- at the default parameters
(levels 4, search 2, smooth 8, reach 0, agree 8).  Everything is already on the device.

    whole      temporal_fill_checked against the unchanged temporal_fill on the same clip in the same process, alternately:
               featurebench.wall, the median of `iters` runs and their min..max, and the ratio.  featurebench.events around
               each call as well.
    backward   what a backward step costs more than the plain one: the difference of the two calls' event times over the
               F - 1 backward steps (everything else in the two calls is the same launches), next to one lp_tfill_carry_pair and
               one lp_tfill_carry (nearer = 1) launch on the middle frame, each timed between two events with the frame's planes
               put back before every launch.  A kernel trace of `--job checked` / `--job plain` gives the time per kernel itself.
    agreement  on these clips nothing moves through the hole: the disputed pixels, and the elements of filled / remaining / source
               that differ from the plain call's.
    second     clips of the same size with a second object, a textured square that falls through the masked disc's path and is
               not masked itself, once with the disc of the timed clips (most of its path is covered either from the first frame
               or until the last, so one direction only reaches it) and once with a disc of 5 / 12 the radius (most pixels have
               two witnesses): per form the pixels filled, disputed and wrong.  Wrong: a borrowed pixel further than 8 grey
               levels, in any channel, from the clip drawn without the disc.

    python scripts/bench_temporal_fill_checked.py [--iters 5] [--warmup 1] [--case clip]
    python scripts/bench_temporal_fill_checked.py --job checked --case clip --iters 3     # the body of a kernel-trace run
"""
from __future__ import annotations

import featurebench as fb

import bench_propagate as single  # the cases
import bench_temporal_fill as plain  # the workloads

LEVELS, SEARCH, SMOOTH, REACH, AGREE = plain.LEVELS, plain.SEARCH, plain.SMOOTH, plain.REACH, 8
WRONG = 8 / 255
DISCS = (5, 12)                                                         # the second-object clips: the disc's radius is min(H, W) over these


def second_object_job(case, dev, divisor):
    """A clip of the case's size in three layers: a textured background that pans one pixel per frame, over it a textured square
    of a third of the shorter side that falls 3 pixels per frame and is not masked, and on top the masked subject, a constant
    disc of radius min(H, W) / `divisor` on bench_temporal_fill's path, which the square meets in the middle of the clip.  `clean`
    is the clip without the disc."""
    import torch
    import torch.nn.functional as Fn
    F, H, W = single.CASES[case]
    g = torch.Generator(device="cpu").manual_seed(1)

    def texture(h, w, cell):                                          # smooth noise [h, w, 3] in 0..1
        n = torch.rand(1, 3, h // cell + 2, w // cell + 2, generator=g)
        return Fn.interpolate(n, size=(h, w), mode="bilinear", align_corners=False)[0].permute(1, 2, 0).to(dev)
    bg = 0.5 * texture(H + F, W + F, 4) + 0.5 * texture(H + F, W + F, 32)
    side = min(H, W) // 3
    square = texture(side, side, 2)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    r, cy0, cx0 = min(H, W) / divisor, H / 3, W / 4
    clean = torch.empty(F, H, W, 3, device=dev)
    for t in range(F):
        clean[t] = bg[t // 2:t // 2 + H, F - t:F - t + W]
        y0 = int(cy0 + 1.5 * (F // 2) - side / 2 + 3 * (t - F // 2))
        x0 = int(cx0 + 4.0 * (F // 2) - side / 2)
        ys, xs = slice(max(y0, 0), min(y0 + side, H)), slice(max(x0, 0), min(x0 + side, W))
        if ys.start < ys.stop and xs.start < xs.stop:
            clean[t, ys, xs] = square[ys.start - y0:ys.stop - y0, xs.start - x0:xs.stop - x0]
    disc = torch.stack([(yy - cy0 - 1.5 * t) ** 2 + (xx - cx0 - 4.0 * t) ** 2 <= r * r for t in range(F)])
    grown = torch.stack([(yy - cy0 - 1.5 * t) ** 2 + (xx - cx0 - 4.0 * t) ** 2 <= (r + plain.GROW) ** 2 for t in range(F)])
    return {"case": case, "shape": (F, H, W), "clean": clean, "images": torch.where(disc[..., None], 0.5, clean), "masks": grown.float()}


def second_object_counts(case, dev, divisor):
    """Filled, disputed and wrong pixels of both forms on the clip with the second object."""
    from lanpaint_amd import temporal_fill as tf, temporal_fill_checked as tc
    job = second_object_job(case, dev, divisor)
    images, masks, clean = job["images"], job["masks"], job["clean"]
    res = {"disc_radius": round(min(job["shape"][1:]) / divisor, 1), "masked_pixels": int((masks >= 0.5).sum())}
    for name, got in (("plain", tf.temporal_fill(images, masks, LEVELS, SEARCH, SMOOTH, REACH)),
                      ("checked", tc.temporal_fill_checked(images, masks, LEVELS, SEARCH, SMOOTH, REACH, AGREE))):
        filled, source = got[0], got[2]
        borrowed = (masks >= 0.5) & (source >= 0)
        wrong = borrowed & ((filled - clean).abs().amax(dim=-1) > WRONG)
        res[name] = {"filled": int(borrowed.sum()), "disputed": int((source == -2).sum()), "wrong": int(wrong.sum())}
        if name == "checked":
            res[name].update(verified=int((got[3] == 2).sum()), wrong_and_verified=int((wrong & (got[3] == 2)).sum()),
                             one_witness=int((got[3] == 1).sum()), wrong_and_one_witness=int((wrong & (got[3] == 1)).sum()))
    return res


def backward_alone(job, reps):
    """One backward step of the middle frame in both forms, every pixel of both neighbours with an origin, the frame's planes put
    back before every launch: (pair ms, plain ms)."""
    import torch
    from lanpaint_amd import propagate, temporal_fill as tf, temporal_fill_checked as tc
    F, H, W = job["shape"]
    images, t, dev = job["images"], F // 2, job["images"].device
    luma = propagate.luma_pyramids(images[t - 1:t + 2], LEVELS)
    known = tf.known_pyramids(job["masks"][t - 1:t + 2], 3, LEVELS)
    vec = tf.step_fields(luma, known, [(1, 0), (1, 2)], H, W, LEVELS, SEARCH, SMOOTH)
    bits = [propagate.level_view(known, H, W, 0)[i] for i in (0, 1, 2)]
    filled, source = images.clone(), torch.full((F, H, W), -1, dtype=torch.int32, device=dev)
    remaining, witnesses = torch.ones((F, H, W), device=dev), torch.zeros((F, H, W), dtype=torch.int32, device=dev)
    out = tf.new_state(H, W, dev)
    own = torch.stack(torch.meshgrid(16 * torch.arange(H, device=dev), 16 * torch.arange(W, device=dev), indexing="ij"), dim=-1).int()
    past, future = (torch.full((H, W), t - 1, dtype=torch.int32, device=dev), own), (torch.full((H, W), t + 1, dtype=torch.int32, device=dev), own)
    tf.carry(vec[0], bits[1], bits[0], past, images, filled, source, remaining, t, t - 1, 0, False, out)     # A: from frame t - 1
    keep = filled[t].clone(), source[t].clone(), remaining[t].clone()
    runs = {"pair": lambda: tc.carry_pair(vec[1], bits[1], bits[2], future, images, filled, source, remaining, witnesses, t, 0, AGREE, out),
            "plain": lambda: tf.carry(vec[1], bits[1], bits[2], future, images, filled, source, remaining, t, t + 1, 0, True, out)}
    ms = {}
    for name, run in runs.items():
        times = []
        for _ in range(reps + 1):
            filled[t], source[t], remaining[t] = keep
            times.append(fb.events(run))
        ms[name] = fb.median(times[1:])
    return ms["pair"], ms["plain"]


def measure(job, iters, warmup, reps):
    from lanpaint_amd import temporal_fill as tf, temporal_fill_checked as tc
    F, H, W = job["shape"]
    images, masks = job["images"], job["masks"]
    new = lambda: tc.temporal_fill_checked(images, masks, LEVELS, SEARCH, SMOOTH, REACH, AGREE)     # noqa: E731
    old = lambda: tf.temporal_fill(images, masks, LEVELS, SEARCH, SMOOTH, REACH)                    # noqa: E731
    got, base = new(), old()
    again = fb.differing(new(), got)
    disputed = int((got[2] == -2).sum())
    from_plain = fb.differing(got[:3], base)
    verified, one = int((got[3] == 2).sum()), int((got[3] == 1).sum())
    del got, base
    # alternating: the two share whatever else the host does
    s = fb.series([("new", new, fb.wall), ("old", old, fb.wall), ("new_events", new), ("old_events", old)], iters, warmup)
    new_ms, old_ms, new_ev, old_ev = s.values()
    med = fb.median
    pair_ms, carry_ms = backward_alone(job, reps)
    return {"case": job["case"], "frames_height_width": [F, H, W], "levels": LEVELS, "search": SEARCH, "smooth": SMOOTH, "reach": REACH,
            "agree": AGREE,
            "checked_wall_ms": round(med(new_ms), 3), "checked_wall_min_max_ms": fb.summary(new_ms, 3)[1],
            "plain_wall_ms": round(med(old_ms), 3), "plain_wall_min_max_ms": fb.summary(old_ms, 3)[1],
            "checked_over_plain": round(med(new_ms) / med(old_ms), 3),
            "checked_events_ms": round(med(new_ev), 3), "plain_events_ms": round(med(old_ev), 3),
            "checked_over_plain_events": round(med(new_ev) / med(old_ev), 3),
            "extra_ms_per_backward_step_by_difference": round((med(new_ev) - med(old_ev)) / (F - 1), 5),
            "pair_alone_ms": round(pair_ms, 5), "plain_backward_carry_alone_ms": round(carry_ms, 5), "stage_reps": reps,
            "disputed_pixels": disputed, "verified_pixels": verified, "one_witness_pixels": one,
            "elements_differing_from_the_plain_call": from_plain, "elements_differing_between_two_calls": again,
            "second_object": [second_object_counts(job["case"], images.device, divisor) for divisor in DISCS]}


def main():
    ap = fb.parser(single.CASES, ("checked", "plain"), iters=5, warmup=1)
    ap.add_argument("--reps", type=int, default=20, help="launches per stage timing")
    a = ap.parse_args()
    dev = fb.device()
    import torch
    from lanpaint_amd import temporal_fill as tf, temporal_fill_checked as tc
    results = []
    for case in ((a.case,) if a.case else tuple(single.CASES)):
        job = plain.make_job(case, dev)
        if a.job:
            body = {"checked": lambda: tc.temporal_fill_checked(job["images"], job["masks"], LEVELS, SEARCH, SMOOTH, REACH, AGREE),
                    "plain": lambda: tf.temporal_fill(job["images"], job["masks"], LEVELS, SEARCH, SMOOTH, REACH)}[a.job]
            fb.untimed(body, a.warmup + a.iters)
        else:
            results.append(measure(job, a.iters, a.warmup, a.reps))
        del job
        torch.cuda.empty_cache()
    if not a.job:
        fb.emit("video_temporal_fill_checked", a, results)


if __name__ == "__main__":
    main()
