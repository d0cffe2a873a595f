#!/usr/bin/env python3
"""Video mask stabilize benchmark (lanpaint_amd.stabilize on the HIP device): one JSON line.

Two workloads, everything already on the device, at the radius pairs (median, smooth) = (1, 2) and (3, 8), grow 0, feather 0:

    clip    81 frames of 1280 x 720: a disc that drifts and jitters, two empty frames and a stray blob
    square  16 frames of 1024 x 1024, the same

    whole     stabilize.stabilize_masks: the EDT per chunk of frames, the fold into q, the temporal launch
    edt       stabilize.signed_d2 alone: videomask.keyframe_edt and lp_mask_signed_d2 (what the whole spends before the new launch)
    temporal  stabilize.stabilize_q alone: the one fused lp_mask_stabilize launch on a q that is already there
    torch     the temporal rule in torch operators on the same q and device: the median window by torch.stack of clamped
              index_select views and torch.sort, sign * sqrt in fp64, clamp, the binomial sum as a running weighted sum, the
              threshold.  Its result is compared with the launch's; the count of differing elements is printed.
    clone     torch.clone of q: one int32 read and one written per pixel and frame, F * H * W * 8 bytes -- exactly what the rule
              has to move in the temporal launch -- at the copy rate this process reaches on this very tensor, in the same run.

    python scripts/bench_stabilize.py [--iters 10] [--warmup 2] [--case clip]
    python scripts/bench_stabilize.py --job temporal --case clip --iters 10      # the body of a rocprofv3 --kernel-trace run

Time: featurebench.events per call; every iteration runs temporal, torch, temporal, torch, clone, edt, whole.  The clip's q and
out together are 597 MB and do not fit the 256 MiB Infinity Cache; the square's are 134 MB and do.
"""
from __future__ import annotations

import math

import featurebench as fb

CASES = {"clip": (81, 720, 1280), "square": (16, 1024, 1024)}
PAIRS = ((1, 2), (3, 8))
INFINITY_CACHE_BYTES = 256 << 20


def make_job(case, dev):
    import torch
    from lanpaint_amd import stabilize
    F, H, W = CASES[case]
    g = torch.Generator(device="cpu").manual_seed(0)
    jitter = torch.randn(F, 3, generator=g)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    mask = torch.empty(F, H, W, device=dev)
    for t in range(F):
        cy = H / 2 + 0.5 * t + 1.5 * float(jitter[t, 0])
        cx = W / 3 + 2.0 * t + 1.5 * float(jitter[t, 1])
        mask[t] = ((yy - cy) ** 2 + (xx - cx) ** 2 <= (min(H, W) / 4 + 2.0 * float(jitter[t, 2])) ** 2).float()
    mask[F // 3] = 0.0
    mask[2 * F // 3] = 0.0
    mask[F // 2, 5:15, W - 30:W - 15] = 1.0
    return {"case": case, "mask": mask, "q": stabilize.signed_d2(mask)}


def torch_temporal(q, median, smooth):
    """Stages 2 to 5 at grow = feather = 0 in torch operators: q int32 [F, H, W] -> fp32 [F, H, W]."""
    import torch
    F = q.shape[0]
    t = torch.arange(F, device=q.device)
    window = torch.stack([q.index_select(0, (t + k).clamp(0, F - 1)) for k in range(-median, median + 1)])
    qm = torch.sort(window, dim=0).values[median]
    del window
    s = (torch.sign(qm).double() * torch.sqrt(qm.abs().double())).clamp(-64.0, 64.0)
    del qm
    acc = torch.zeros_like(s)
    for k in range(-smooth, smooth + 1):
        acc += float(math.comb(2 * smooth, smooth + k)) * s.index_select(0, (t + k).clamp(0, F - 1))
    return (acc / float(4 ** smooth) > 0).float()


def jobs(pair):
    from lanpaint_amd import stabilize
    median, smooth = pair
    return {"temporal": lambda j: stabilize.stabilize_q(j["q"], median, smooth),
            "torch": lambda j: torch_temporal(j["q"], median, smooth),
            "clone": lambda j: j["q"].clone(),
            "edt": lambda j: stabilize.signed_d2(j["mask"]),
            "whole": lambda j: stabilize.stabilize_masks(j["mask"], median, smooth)}


def run(job, pair, iters, warmup, only=None):
    fn = {name: (lambda f=f: f(job)) for name, f in jobs(pair).items()}
    order = [("temporal_a", "temporal"), ("torch_a", "torch"), ("temporal_b", "temporal"), ("torch_b", "torch"), ("clone", "clone"),
             ("edt", "edt"), ("whole", "whole")]
    if only:
        order = [(only, only)]
    return fb.series([(tag, fn[name]) for tag, name in order], iters, warmup)


def measure(job, pair, iters, warmup):
    import torch
    fn = jobs(pair)
    got, eager = fn["temporal"](job), fn["torch"](job)
    differing = fb.differing(got, eager)
    changed = int((got != (job["mask"] >= 0.5).float()).sum())
    del got, eager
    torch.cuda.empty_cache()
    s = run(job, pair, iters, warmup)
    med = fb.median
    F, H, W = CASES[job["case"]]
    moved = F * H * W * 8
    temporal, eager = med(s["temporal_a"] + s["temporal_b"]), med(s["torch_a"] + s["torch_b"])
    clone, edt, whole = med(s["clone"]), med(s["edt"]), med(s["whole"])
    return {"case": job["case"], "frames_height_width": [F, H, W], "median": pair[0], "smooth": pair[1],
            "elements_differing_from_torch": differing, "elements_changed_by_the_filter": changed,
            "whole_ms": round(whole, 4), "edt_ms": round(edt, 4), "edt_share_of_whole": round(edt / whole, 3),
            "temporal_ms": round(temporal, 4), "torch_ms": round(eager, 4), "clone_ms": round(clone, 4),
            "torch_over_temporal": round(eager / temporal, 2), "temporal_over_clone": round(temporal / clone, 2),
            "temporal_min_max_ms": fb.summary(s["temporal_a"] + s["temporal_b"])[1],
            "torch_min_max_ms": fb.summary(s["torch_a"] + s["torch_b"])[1], "whole_min_max_ms": fb.summary(s["whole"])[1],
            "temporal_spread": fb.spread(s["temporal_a"], s["temporal_b"]), "torch_spread": fb.spread(s["torch_a"], s["torch_b"]),
            "required_bytes": moved, "fits_infinity_cache": moved <= INFINITY_CACHE_BYTES,
            "temporal_tb_per_s": round(moved / (temporal * 1e-3) / 1e12, 3), "clone_tb_per_s": round(moved / (clone * 1e-3) / 1e12, 3)}


def main():
    a = fb.parser(CASES, ("temporal", "torch", "edt", "whole")).parse_args()
    dev = fb.device()
    import torch
    results = []
    for case in ((a.case,) if a.case else tuple(CASES)):
        job = make_job(case, dev)
        for pair in PAIRS:
            if a.job:
                run(job, pair, a.iters, a.warmup, only=a.job)
            else:
                results.append(measure(job, pair, a.iters, a.warmup))
            torch.cuda.empty_cache()
        del job
        torch.cuda.empty_cache()
    if not a.job:
        fb.emit("mask_stabilize", a, results,
                temporal_faster_than_torch_in_every_case=all(r["torch_over_temporal"] > 1.0 for r in results))


if __name__ == "__main__":
    main()
