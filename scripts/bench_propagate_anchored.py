#!/usr/bin/env python3
"""Anchored video mask propagate benchmark (lanpaint_amd.propagate_anchored on the HIP device): one JSON line.

The two workloads of scripts/bench_propagate.py at the default parameters (levels 4, search 2, smooth 8, anchor 2), key frame 0,
everything already on the device:

    clip    81 frames of 1280 x 720 x 3
    square  16 frames of 1024 x 1024 x 3

    whole     propagate_anchored.propagate_masks_anchored against propagate.propagate_masks on the same clip in the same process,
              alternating, each with featurebench.wall.  Their ratio is the figure that
              matters; from the launch counts (2 levels + 4 against 2 levels + 1 a step) one would guess 12 / 9.
    launches  the entry names of one step of either form, counted from the modules' own launches.
    stages    lp_prop_anchor_match alone on the buffers of the clip's first step, featurebench.events over `reps` back-to-back
              calls, next to the step's other launches timed the same way.
    drift     the last frame's IoU of both forms against the truth on a clip of the same size built as tests/anchor_clips.py
              builds its own: a textured disc that moves (0.23, 0.61) pixel per frame over a still textured background, bilinear
              sampling, Gaussian noise of 0.01.  This is the clip the form is for; the timed clip's disc moves by whole pixels.

    python scripts/bench_propagate_anchored.py [--iters 5] [--warmup 1] [--case clip] [--reps 50]
"""
from __future__ import annotations

import featurebench as fb

import bench_propagate as base  # the clip

LEVELS, SEARCH, SMOOTH, ANCHOR = base.LEVELS, base.SEARCH, base.SMOOTH, 2


def subpixel_job(case, dev, vy=0.23, vx=0.61, noise=0.01):
    """tests/anchor_clips.py's subpixel_clip at a workload's size, built on the device: (images [F, H, W, 3], truth bool
    [F, H, W])."""
    import torch
    F, H, W = base.CASES[case]
    g = torch.Generator(device="cpu").manual_seed(36)

    def tex(h, w):
        a = torch.rand(h, w, generator=g, dtype=torch.float64).to(dev)
        for ax in (0, 1):
            a = (torch.roll(a, -1, ax) + 2 * a + torch.roll(a, 1, ax)) / 4
        return (a - a.min()) / (a.max() - a.min())
    bg, subj = tex(H, W), tex(2 * H, 2 * W)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    R, cy0, cx0 = min(H, W) / 5, 0.35 * H, 0.3 * W
    images = torch.empty(F, H, W, 3, device=dev)
    truth = torch.empty(F, H, W, dtype=torch.bool, device=dev)
    gd = torch.Generator(device=dev).manual_seed(37)
    for t in range(F):
        inside = (yy - cy0 - vy * t) ** 2 + (xx - cx0 - vx * t) ** 2 <= R * R
        sy, sx = yy - vy * t + H / 2, xx - vx * t + W / 2
        iy, ix = sy.floor().long(), sx.floor().long()
        fy, fx = sy - iy, sx - ix
        s = (1 - fy) * ((1 - fx) * subj[iy, ix] + fx * subj[iy, ix + 1]) + fy * ((1 - fx) * subj[iy + 1, ix] + fx * subj[iy + 1, ix + 1])
        f = torch.where(inside, s, bg) + noise * torch.randn(H, W, generator=gd, device=dev, dtype=torch.float64)
        images[t] = f.float()[..., None]
        truth[t] = inside
    return images, truth


def iou(a, b):
    return float((a & b).sum()) / max(int((a | b).sum()), 1)


def drift(case, dev):
    """The last frame's IoU of the plain and of the anchored form on the sub-pixel clip, and the anchored form's worst frame."""
    from lanpaint_amd import propagate, propagate_anchored as pa
    images, truth = subpixel_job(case, dev)
    mask = truth[0].float()
    plain = propagate.propagate_masks(images, mask, 0, LEVELS, SEARCH, SMOOTH) >= 0.5
    anchored = pa.propagate_masks_anchored(images, mask, 0, LEVELS, SEARCH, SMOOTH, ANCHOR) >= 0.5
    F = truth.shape[0]
    return {"plain_last_iou": round(iou(plain[-1], truth[-1]), 4), "anchored_last_iou": round(iou(anchored[-1], truth[-1]), 4),
            "plain_worst_iou": round(min(iou(plain[t], truth[t]) for t in range(F)), 4),
            "anchored_worst_iou": round(min(iou(anchored[t], truth[t]) for t in range(F)), 4)}


def stage_times(job, reps):
    """The step's launches alone on the first step's buffers: ms per call."""
    import torch
    from lanpaint_amd import propagate, propagate_anchored as pa
    F, H, W = job["shape"]
    out = {}
    pyr = propagate.luma_pyramids(job["images"][:2], LEVELS)
    mpyr, _ = propagate.key_mask(job["mask"], LEVELS)
    step = propagate.Step(H, W, LEVELS, SEARCH, SMOOTH, job["images"].device, rematch=(pa.anchor_field, ANCHOR, SMOOTH))
    step.field_of(pyr[0], pyr[1], mpyr)
    for lv in range(LEVELS - 1, -1, -1):
        parent = None if lv == LEVELS - 1 else step.field[lv + 1]
        out[f"match_level{lv}"] = fb.events(lambda: propagate.match_level(pyr[0], pyr[1], mpyr, H, W, LEVELS, lv, SEARCH, SMOOTH, parent,
                                                                            step.raw[lv], step.valid[lv]), reps)
        out[f"fill_level{lv}"] = fb.events(lambda: propagate.fill_median(step.raw[lv], step.valid[lv], step.field[lv]), reps)
    key_bits = propagate.level_view(mpyr, H, W, 0)[0]
    out["advance"] = fb.events(lambda: propagate.advance(step.field[0], None, key_bits, LEVELS, step.raw_pos, step.code, step.raw_mpyr), reps)
    luma_t, luma_k = (propagate.level_view(pyr[i:i + 1], H, W, 0)[0] for i in (1, 0))
    bits = propagate.level_view(step.raw_mpyr, H, W, 0)[0]
    vec, valid = (torch.empty_like(t) for t in (step.raw[0], step.valid[0]))
    out["anchor_match"] = fb.events(lambda: pa.anchor_field(step.raw_pos, luma_t, luma_k, bits, ANCHOR, SMOOTH, vec, valid), reps)
    e = torch.empty_like(step.field[0])
    out["anchor_fill"] = fb.events(lambda: propagate.fill_median(vec, valid, e), reps)
    o = torch.empty((H, W), dtype=torch.float32, device=bits.device)
    out["anchor_advance"] = fb.events(lambda: propagate.advance(e, step.raw_pos, key_bits, LEVELS, step.pos[0], o, step.mpyr[0]), reps)
    torch.cuda.synchronize()
    return out, int(valid.sum()), valid.numel()


def measure(job, iters, warmup, reps):
    from lanpaint_amd import propagate, propagate_anchored as pa
    F, H, W = job["shape"]
    new = lambda: pa.propagate_masks_anchored(job["images"], job["mask"], 0, LEVELS, SEARCH, SMOOTH, ANCHOR)      # noqa: E731
    old = lambda: propagate.propagate_masks(job["images"], job["mask"], 0, LEVELS, SEARCH, SMOOTH)               # noqa: E731
    got, plain = new(), old()
    differing_again = fb.differing(new(), got)
    skip = ("lp_prop_luma", "lp_prop_key_mask")
    small = job["images"][:2]
    step_new = [n for n in fb.count_launches(lambda: pa.propagate_masks_anchored(small, job["mask"], 0, LEVELS, SEARCH, SMOOTH, ANCHOR),
                                               pa, propagate) if n not in skip]
    step_old = [n for n in fb.count_launches(lambda: propagate.propagate_masks(small, job["mask"], 0, LEVELS, SEARCH, SMOOTH)) if n not in skip]
    truth = job["truth"]
    ious = {"anchored_last_iou": round(iou(got[-1] >= 0.5, truth), 4), "plain_last_iou": round(iou(plain[-1] >= 0.5, truth), 4),
            "elements_differing_from_plain": fb.differing(got, plain)}
    del got, plain
    # alternating: the two share whatever else the host does
    new_ms, old_ms = fb.series([("new", new), ("old", old)], iters, warmup, timer=fb.wall).values()
    stages, valid, blocks = stage_times(job, reps)
    med = fb.median
    return {"case": job["case"], "frames_height_width": [F, H, W], "levels": LEVELS, "search": SEARCH, "smooth": SMOOTH, "anchor": ANCHOR,
            "anchored_wall_ms": round(med(new_ms), 3), "anchored_wall_min_max_ms": fb.summary(new_ms, 3)[1],
            "plain_wall_ms": round(med(old_ms), 3), "plain_wall_min_max_ms": fb.summary(old_ms, 3)[1],
            "anchored_over_plain": round(med(new_ms) / med(old_ms), 3),
            "launches_per_step": [len(step_new), len(step_old)], "step_entries": step_new,
            "stage_ms": {k: round(v, 5) for k, v in stages.items()}, "stage_reps": reps,
            "anchor_match_ms": round(stages["anchor_match"], 5),
            "new_launches_ms_per_step": round(stages["anchor_match"] + stages["anchor_fill"] + stages["anchor_advance"], 5),
            "first_step_blocks_valid": [valid, blocks], "timed_clip": ious, "elements_differing_between_two_calls": differing_again}


def main():
    ap = fb.parser(base.CASES, iters=5, warmup=1)
    ap.add_argument("--reps", type=int, default=50, help="back-to-back calls per stage timing")
    ap.add_argument("--no-drift", action="store_true", help="skip the sub-pixel clip's IoU pair")
    a = ap.parse_args()
    dev = fb.device()
    import torch
    results = []
    for case in ((a.case,) if a.case else tuple(base.CASES)):
        job = base.make_job(case, dev)
        r = measure(job, a.iters, a.warmup, a.reps)
        del job
        torch.cuda.empty_cache()
        if not a.no_drift:
            r["subpixel_clip"] = drift(case, dev)
            torch.cuda.empty_cache()
        results.append(r)
    fb.emit("mask_propagate_anchored", a, results)


if __name__ == "__main__":
    main()
