#!/usr/bin/env python3
"""Anchored occlusion-aware video mask propagate benchmark (lanpaint_amd.propagate_anchored_visible on the HIP device): one JSON line.

The two workloads of scripts/bench_propagate_anchored.py at the default parameters (levels 4, search 2, smooth 8, anchor 2,
occlusion 16), key frame 0, everything already on the device:

    clip    81 frames of 1280 x 720 x 3
    square  16 frames of 1024 x 1024 x 3

    whole     propagate_masks_anchored_visible against propagate_masks_anchored and propagate_masks_visible on the same clip in
              the same process, alternating, each with featurebench.wall, medians.  From the
              launch counts (2 levels + 6 against 2 levels + 4 and 2 levels + 3 a step) one would guess the anchored call plus the
              visible form's two launches a step.
    launches  the entry names of one step, counted from the modules' own launches.
    gate      lp_prop_anchor_match_gated alone against lp_prop_anchor_match alone on the buffers of the clip's first step,
              featurebench.events over `reps` back-to-back calls, alternating `rounds` times, medians; the blocks the gate shut.
              --launches-only makes these launches and nothing else to time, at anchor 2 and 7, for a kernel trace of its own.
    torch     the same rule in torch operators on the first `--torch-frames` frames: its time, the module's on the same frames,
              and the number of elements in which the two differ, which must be 0.
    occluded  the last frame's and the worst frame's whole-subject IoU, iou((mask + hidden) >= 0.5, truth), of the three forms on
              the sub-pixel clip of scripts/bench_propagate_anchored.py with a static textured bar of W / 20 columns in the
              subject's way.  This is the clip the form is for; the timed clip's disc moves by whole pixels behind nothing.

    python scripts/bench_propagate_anchored_visible.py [--iters 5] [--warmup 1] [--case clip] [--reps 50] [--torch-frames 4]
"""
from __future__ import annotations

import json

import featurebench as fb

import bench_propagate as base  # the clip, the plain rule in torch
import bench_propagate_anchored as anchored  # the sub-pixel clip
import bench_propagate_visible as visible  # the visible rule in torch

LEVELS, SEARCH, SMOOTH, ANCHOR, OCCLUSION = base.LEVELS, base.SEARCH, base.SMOOTH, 2, 16


# ---- the same rule in torch operators ----------------------------------------------------------------------------------------------------
def torch_gated_field(K, Yt, m, R, smooth, occlusion):
    """lp_prop_anchor_match_gated in torch operators: (vec, valid, gated).  The match is the plain rule's at level 0; the winner
    before the sub-pixel step is found again from the keys, and lp_prop_visible's statistic is taken there."""
    import torch
    vec, live = base.torch_match(K, Yt, m, None, R, smooth, True)
    h, w = K.shape
    dev = K.device
    gh, gw = live.shape
    n = 2 * R + 1
    r = torch.arange(16, device=dev)
    ys = (torch.arange(gh, device=dev)[:, None] * 8 - 4 + r[None, :])[:, None, :, None]
    xs = (torch.arange(gw, device=dev)[:, None] * 8 - 4 + r[None, :])[None, :, None, :]
    inside = (ys >= 0) & (ys < h) & (xs >= 0) & (xs < w)
    flat = ys.clamp(0, h - 1) * w + xs.clamp(0, w - 1)
    mm = m.reshape(-1)[flat] * inside
    win = K.reshape(-1)[flat]
    keys = torch.empty(n * n, gh, gw, dtype=torch.long, device=dev)
    for oy in range(-R, R + 1):
        for ox in range(-R, R + 1):
            idx, dist = (oy + R) * n + ox + R, abs(oy) + abs(ox)
            t = Yt.reshape(-1)[(ys + oy).clamp(0, h - 1) * w + (xs + ox).clamp(0, w - 1)]
            keys[idx] = ((((win - t).abs() * mm).sum(dim=(2, 3)) + smooth * dist) << 12) | (dist << 8) | idx
    best = keys.min(dim=0).values & 255
    oy, ox = (base._floor_div(best, n) - R)[:, :, None, None], (best % n - R)[:, :, None, None]
    dd = Yt.reshape(-1)[(ys + oy).clamp(0, h - 1) * w + (xs + ox).clamp(0, w - 1)] - win
    cnt = mm.sum(dim=(2, 3))
    D = (dd * mm).sum(dim=(2, 3))
    mu = base._floor_div(2 * D + cnt, (2 * cnt).clamp(min=1)).clamp(-32, 32)
    Rs = ((dd - mu[:, :, None, None]).abs() * mm).sum(dim=(2, 3))
    gated = live & (Rs > occlusion * cnt)
    return torch.where(gated[..., None], torch.zeros_like(vec), vec), live & ~gated, gated.long()


def torch_propagate_anchored_visible(images, mask, levels=LEVELS, search=SEARCH, smooth=SMOOTH, anchor=ANCHOR, occlusion=OCCLUSION):
    """propagate_masks_anchored_visible with key frame 0 in torch operators: (mask, hidden) fp32 [F, H, W]."""
    import torch
    F, H, W = images.shape[:3]
    key = (mask >= 0.5).long()
    Y = base.torch_luma(images)
    yy, xx = torch.meshgrid(torch.arange(H, device=images.device), torch.arange(W, device=images.device), indexing="ij")
    P, bits = torch.stack([16 * yy, 16 * xx], dim=-1), key
    out, hidden = [key.float()], [torch.zeros_like(key, dtype=torch.float32)]
    src = base._pyr(Y[0], levels, True)
    for t in range(1, F):
        tgt, mp, parent = base._pyr(Y[t], levels, True), base._pyr(bits, levels, False), None
        for lv in range(levels - 1, -1, -1):
            parent = base.torch_fill_median(*base.torch_match(src[lv], tgt[lv], mp[lv], parent, search, smooth, lv == 0))
        P1, c1 = base.torch_advance(P, parent, key)
        K = (base._bil(Y[0], P1[..., 0], P1[..., 1]) + 128) >> 8
        vec, valid, _ = torch_gated_field(K, Y[t], (c1 >= 128).long(), anchor, smooth, occlusion)
        P, c = base.torch_advance(P1, base.torch_fill_median(vec, valid), key)
        flags = visible.torch_visible_flags(Y[t], Y[0], P, (c >= 128).long(), occlusion)
        cv = (c * visible.torch_weight(flags, H, W) + 128) >> 8
        out.append(cv.float() / 256.0)
        hidden.append((c - cv).float() / 256.0)
        bits, src = (cv >= 128).long(), tgt
    return torch.stack(out), torch.stack(hidden)


# ---- timing ------------------------------------------------------------------------------------------------------------------------------
def gate_times(job, reps, rounds, anchor=ANCHOR):
    """The gated and the ungated launch alone on the first step's buffers, alternating: median ms per call of each, and the
    first step's (gated, live, all) block counts."""
    import torch
    from lanpaint_amd import propagate, propagate_anchored as pa, propagate_anchored_visible as pav
    F, H, W = job["shape"]
    pyr = propagate.luma_pyramids(job["images"][:2], LEVELS)
    mpyr, _ = propagate.key_mask(job["mask"], LEVELS)
    step = propagate.Step(H, W, LEVELS, SEARCH, SMOOTH, job["images"].device, rematch=(pav.gated_anchor_field, anchor, SMOOTH, OCCLUSION),
                          split=(pav.visible_flags, pav.occlude, OCCLUSION))
    vec = step.field_of(pyr[0], pyr[1], mpyr)
    key_bits = propagate.level_view(mpyr, H, W, 0)[0]
    propagate.advance(vec, None, key_bits, LEVELS, step.raw_pos, step.code, step.raw_mpyr)
    luma_t, luma_k = (propagate.level_view(pyr[i:i + 1], H, W, 0)[0] for i in (1, 0))
    bits = propagate.level_view(step.raw_mpyr, H, W, 0)[0]
    raw, valid = torch.empty_like(step.raw[0]), torch.empty_like(step.valid[0])
    gated_fn = lambda: pav.gated_anchor_field(step.raw_pos, luma_t, luma_k, bits, anchor, SMOOTH, OCCLUSION, step.raw[0],   # noqa: E731
                                              step.valid[0], step.gated)
    plain_fn = lambda: pa.anchor_field(step.raw_pos, luma_t, luma_k, bits, anchor, SMOOTH, raw, valid)                      # noqa: E731
    gated_ms, plain_ms = fb.series([("gated", gated_fn), ("plain", plain_fn)], rounds, 1, timer=lambda f: fb.events(f, reps)).values()
    same = bool(torch.equal(torch.where(step.gated != 0, 0, valid), step.valid[0]))
    return fb.median(gated_ms), fb.median(plain_ms), [int(step.gated.sum()), int(valid.sum()), valid.numel()], same


def occluded(case, dev):
    """Whole-subject IoU (last frame, worst frame) of the three forms on the sub-pixel clip with a static bar in the subject's way."""
    import torch
    from lanpaint_amd import propagate_anchored as pa, propagate_anchored_visible as pav, propagate_visible as pv
    images, truth = anchored.subpixel_job(case, dev)
    F, H, W = truth.shape
    x0 = int(0.3 * W + min(H, W) / 5 + 0.2 * W / 20)                   # just right of the disc on the key frame
    g = torch.Generator(device="cpu").manual_seed(99)
    bar = torch.rand(H, W // 20, generator=g).to(dev)
    for ax in (0, 1):
        bar = (torch.roll(bar, -1, ax) + 2 * bar + torch.roll(bar, 1, ax)) / 4
    images[:, :, x0:x0 + W // 20, :] = ((bar - bar.min()) / (bar.max() - bar.min()))[None, :, :, None]
    mask = truth[0].float()
    zero = torch.zeros_like(mask)[None]

    def both(m, h):
        v = [anchored.iou((m[t] + h[t if h.shape[0] > 1 else 0]) >= 0.5, truth[t]) for t in range(1, F)]
        return [round(v[-1], 4), round(min(v), 4)]
    behind = max(float((truth[t, :, x0:x0 + W // 20]).sum()) / float(truth[t].sum()) for t in range(F))
    return {"bar_columns": [x0, x0 + W // 20], "largest_part_of_the_subject_behind_the_bar": round(behind, 3),
            "new_last_worst_iou": both(*pav.propagate_masks_anchored_visible(images, mask, 0, LEVELS, SEARCH, SMOOTH, ANCHOR, OCCLUSION)),
            "anchored_last_worst_iou": both(pa.propagate_masks_anchored(images, mask, 0, LEVELS, SEARCH, SMOOTH, ANCHOR), zero),
            "visible_last_worst_iou": both(*pv.propagate_masks_visible(images, mask, 0, LEVELS, SEARCH, SMOOTH, OCCLUSION))}


def measure(job, iters, warmup, torch_frames, reps, rounds):
    from lanpaint_amd import propagate, propagate_anchored as pa, propagate_anchored_visible as pav, propagate_visible as pv
    F, H, W = job["shape"]
    images, mask = job["images"], job["mask"]
    new = lambda: pav.propagate_masks_anchored_visible(images, mask, 0, LEVELS, SEARCH, SMOOTH, ANCHOR, OCCLUSION)    # noqa: E731
    anc = lambda: pa.propagate_masks_anchored(images, mask, 0, LEVELS, SEARCH, SMOOTH, ANCHOR)                        # noqa: E731
    vis = lambda: pv.propagate_masks_visible(images, mask, 0, LEVELS, SEARCH, SMOOTH, OCCLUSION)                      # noqa: E731
    got, hid = new()
    differing_again = fb.differing(new(), (got, hid))
    timed = {"new_last_iou": round(anchored.iou((got[-1] + hid[-1]) >= 0.5, job["truth"]), 4), "hidden_mass": round(float(hid.sum()), 1),
             "elements_differing_from_anchored": fb.differing(got, anc())}
    n = min(torch_frames, F)
    small = lambda: pav.propagate_masks_anchored_visible(images[:n], mask, 0, LEVELS, SEARCH, SMOOTH, ANCHOR, OCCLUSION)   # noqa: E731
    eager = lambda: torch_propagate_anchored_visible(images[:n], mask)                                                     # noqa: E731
    differing = fb.differing(eager(), small())
    del got, hid
    skip = ("lp_prop_luma", "lp_prop_key_mask")
    step_new = [e for e in fb.count_launches(lambda: pav.propagate_masks_anchored_visible(images[:2], mask, 0, LEVELS, SEARCH, SMOOTH,
                                                                                             ANCHOR, OCCLUSION), pav, pa, pv, propagate)
                if e not in skip]
    # alternating: the three share whatever else the host does
    fb.untimed(lambda: (new(), anc(), vis()), warmup)
    s = fb.series([("new", new), ("anchored", anc), ("visible", vis), ("torch", eager), ("small", small)], iters, 0, timer=fb.wall)
    new_ms, anc_ms, vis_ms, torch_ms, small_ms = s.values()
    gated_ms, plain_ms, blocks, same = gate_times(job, reps, rounds)
    med = fb.median
    return {"case": job["case"], "frames_height_width": [F, H, W], "levels": LEVELS, "search": SEARCH, "smooth": SMOOTH, "anchor": ANCHOR,
            "occlusion": OCCLUSION,
            "new_wall_ms": round(med(new_ms), 3), "new_wall_min_max_ms": fb.summary(new_ms, 3)[1],
            "anchored_wall_ms": round(med(anc_ms), 3), "anchored_wall_min_max_ms": fb.summary(anc_ms, 3)[1],
            "visible_wall_ms": round(med(vis_ms), 3), "visible_wall_min_max_ms": fb.summary(vis_ms, 3)[1],
            "new_over_anchored": round(med(new_ms) / med(anc_ms), 3), "new_over_visible": round(med(new_ms) / med(vis_ms), 3),
            "launches_per_step": len(step_new), "step_entries": step_new,
            "gated_launch_ms": round(gated_ms, 5), "ungated_launch_ms": round(plain_ms, 5), "gated_over_ungated": round(gated_ms / plain_ms, 3),
            "launch_reps_rounds": [reps, rounds], "first_step_blocks_gated_live_all": blocks,
            "gated_launch_equals_ungated_where_open": same,
            "timed_clip": timed, "elements_differing_between_two_calls": differing_again,
            "torch_frames": n, "torch_ms": round(med(torch_ms), 3), "module_ms_same_frames": round(med(small_ms), 3),
            "torch_over_module": round(med(torch_ms) / med(small_ms), 2), "elements_differing_from_torch": differing}


def main():
    ap = fb.parser(base.CASES, iters=5, warmup=1)
    ap.add_argument("--reps", type=int, default=50, help="back-to-back calls per launch timing")
    ap.add_argument("--rounds", type=int, default=7, help="alternating launch timings, of which the median is taken")
    ap.add_argument("--torch-frames", type=int, default=4)
    ap.add_argument("--no-occluded", action="store_true", help="skip the occluded sub-pixel clip's IoU")
    ap.add_argument("--launches-only", action="store_true",
                    help="the two launches alone at anchor 2 and 7, for a kernel trace: rocprofv3 --kernel-trace --stats -- python ...")
    a = ap.parse_args()
    dev = fb.device()
    import torch
    results = []
    if a.launches_only:
        for case in ((a.case,) if a.case else tuple(base.CASES)):
            job = base.make_job(case, dev, 2)
            for anchor in (2, 7):
                gated_ms, plain_ms, blocks, _ = gate_times(job, a.reps, a.rounds, anchor)
                results.append({"case": case, "anchor": anchor, "gated_launch_ms": round(gated_ms, 5), "ungated_launch_ms": round(plain_ms, 5),
                                "gated_over_ungated": round(gated_ms / plain_ms, 3), "first_step_blocks_gated_live_all": blocks})
        print(json.dumps({"metric": "anchor_match_launches", "unit": "ms", "reps_rounds": [a.reps, a.rounds], "cases": results},
                         separators=(",", ":")))
        return
    for case in ((a.case,) if a.case else tuple(base.CASES)):
        job = base.make_job(case, dev)
        r = measure(job, a.iters, a.warmup, a.torch_frames, a.reps, a.rounds)
        del job
        torch.cuda.empty_cache()
        if not a.no_occluded:
            r["occluded_subpixel_clip"] = occluded(case, dev)
            torch.cuda.empty_cache()
        results.append(r)
    fb.emit("mask_propagate_anchored_visible", a, results)
    if any(r["elements_differing_from_torch"] for r in results):
        raise SystemExit("the module differs from the same rule in torch operators")


if __name__ == "__main__":
    main()
