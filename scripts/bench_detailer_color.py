#!/usr/bin/env python3
"""Detailer colour match benchmark (lanpaint_amd.detail_color on the HIP device): one JSON line.

The workload: 81 decoded crops of 576 x 1024 x 3 against the 81 original crops and an 81-frame crop mask (a disc of radius 150
that drifts across the window), method mean_std, margin 8, smooth 9.  Everything is already on the device.

    hip    detail_color.match(detail, reference, mask, "mean_std", 1.0, 8, 9, 0): lp_color_stats, lp_color_fit, lp_color_apply
    eager  the same mathematics composed from torch operators on the same device: max_pool2d for the keep mask, fp64 masked
           sums, a cumulative-sum window for the pooling, the fit in fp64 tensors, the affine map in fp32.  The yardstick: no
           earlier revision has a colour match to time.
    clone  torch.clone of the detail tensor: the copy rate this process reaches on these very tensors, in the same run.

    python scripts/bench_detailer_color.py [--iters 20] [--warmup 3]
    python scripts/bench_detailer_color.py --job hip --iters 10          # the body of a rocprofv3 --kernel-trace run

Time: featurebench.events per call; every iteration runs hip, eager, hip, eager, then the three HIP stages on their own and
the clone.
Bytes: what the algorithm has to move -- two image reads and one mask read for the statistics, one image read and one write
for the map -- over the time, and that rate over the clone's (one read, one write).
"""
from __future__ import annotations

import featurebench as fb

FRAMES, H, W, C = 81, 576, 1024, 3
RADIUS, MARGIN, SMOOTH, METHOD, STRENGTH = 150, 8, 9, "mean_std", 1.0


def make_job(dev):
    import torch
    g = torch.Generator(device="cpu").manual_seed(0)
    reference = torch.rand(FRAMES, H, W, C, generator=g).to(dev)
    gain = (0.9 + 0.2 * torch.rand(FRAMES, 1, 1, C, generator=g)).to(dev)
    bias = (0.1 * torch.rand(FRAMES, 1, 1, C, generator=g) - 0.05).to(dev)
    detail = reference * gain + bias                               # a different drift per frame and channel
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    mask = torch.zeros(FRAMES, H, W)
    for f in range(FRAMES):
        cx = 300 + 424 * f // (FRAMES - 1)
        mask[f] = ((yy - H // 2) ** 2 + (xx - cx) ** 2 < RADIUS * RADIUS).float()
    return {"detail": detail, "reference": reference, "mask": mask.to(dev)}


def required_bytes():
    image, mask = FRAMES * H * W * C * 4, FRAMES * H * W * 4
    return {"stats": 2 * image + mask, "apply": 2 * image, "match": 4 * image + mask, "clone": 2 * image}


def hip_match(j):
    from lanpaint_amd import detail_color
    return detail_color.match(j["detail"], j["reference"], j["mask"], METHOD, STRENGTH, MARGIN, SMOOTH, 0)


def hip_stats(j):
    from lanpaint_amd import detail_color
    j["stats"] = detail_color.color_stats(j["detail"], j["reference"], j["mask"], MARGIN)
    return j["stats"]


def hip_fit(j):
    from lanpaint_amd import detail_color
    j["coef"] = detail_color.color_fit(j["stats"], METHOD, STRENGTH, SMOOTH, 0)
    return j["coef"]


def hip_apply(j):
    from lanpaint_amd import detail_color
    return detail_color.color_apply(j["detail"], j["coef"])


def clone(j):
    return j["detail"].clone()


def eager_match(j):
    """The rule of lanpaint_amd/detail_color.py in torch operators (mean_std, strength 1, one clip)."""
    import torch
    import torch.nn.functional as F
    d, r, m = j["detail"], j["reference"], j["mask"]
    over = (~(m <= 0.5)).float().unsqueeze(1)
    near = F.max_pool2d(over, 2 * MARGIN + 1, 1, MARGIN)           # padded with -inf: outside the image does not count
    keep = (near == 0).squeeze(1).unsqueeze(-1).double()           # [B, H, W, 1]
    dd, rr = d.double() * keep, r.double() * keep
    n = keep.sum((1, 2))                                           # [B, 1]
    rows = torch.cat([n, dd.sum((1, 2)), rr.sum((1, 2)), (dd * dd).sum((1, 2)), (rr * rr).sum((1, 2))], dim=1)   # [B, 1 + 4 C]
    cs = torch.cat([torch.zeros_like(rows[:1]), rows.cumsum(0)], dim=0)
    f = torch.arange(FRAMES, device=d.device)
    lo, hi = (f - SMOOTH // 2).clamp(min=0), (f + SMOOTH // 2).clamp(max=FRAMES - 1)
    P = cs[hi + 1] - cs[lo]
    N = P[:, :1]
    sd, sr, sdd, srr = (P[:, 1 + k * C: 1 + (k + 1) * C] for k in range(4))
    md, mr = sd / N, sr / N
    vd, vr = sdd / N - md * md, srr / N - mr * mr
    g = torch.where((vd <= 1e-8) | ~(vr >= 0), torch.ones_like(vd), (vr / vd).sqrt().clamp(0.25, 4.0))
    b = mr - g * md
    ok = N >= 64
    gain = torch.where(ok, 1 + STRENGTH * (g - 1), torch.ones_like(g)).float()
    bias = torch.where(ok, STRENGTH * b, torch.zeros_like(b)).float()
    return d * gain[:, None, None, :] + bias[:, None, None, :]


def run(job, iters, warmup, only=None):
    hip, eager, stats, fit, apply, copy = (lambda f=f: f(job) for f in (hip_match, eager_match, hip_stats, hip_fit, hip_apply, clone))
    fns = [("hip_a", hip), ("eager_a", eager), ("hip_b", hip), ("eager_b", eager), ("stats", stats), ("fit", fit), ("apply", apply),
           ("clone", copy)]
    if only:
        fns = [(only + "_a", hip if only == "hip" else eager)]
    return fb.series(fns, iters, warmup)


def main():
    a = fb.parser(jobs=("hip", "eager"), iters=20, warmup=3).parse_args()
    job = make_job(fb.device())
    if a.job:
        run(job, a.iters, a.warmup, only=a.job)
        return
    diff = float((hip_match(job) - eager_match(job)).abs().max())     # the two sides compute the same thing
    s = run(job, a.iters, a.warmup)
    med = fb.median
    need = required_bytes()
    hip, eager = med(s["hip_a"] + s["hip_b"]), med(s["eager_a"] + s["eager_b"])
    clone_tbs = need["clone"] / (med(s["clone"]) * 1e-3) / 1e12
    result = {"image": [FRAMES, H, W, C], "margin": MARGIN, "smooth": SMOOTH,
              "method": METHOD, "max_abs_hip_minus_eager": diff,
              "hip_ms": round(hip, 4), "eager_ms": round(eager, 4), "eager_over_hip": round(eager / hip, 3),
              "hip_min_max_ms": fb.summary(s["hip_a"] + s["hip_b"])[1],
              "eager_min_max_ms": fb.summary(s["eager_a"] + s["eager_b"])[1],
              "hip_spread": fb.spread(s["hip_a"], s["hip_b"]),
              "eager_spread": fb.spread(s["eager_a"], s["eager_b"]),
              "clone_ms": round(med(s["clone"]), 4), "clone_tb_per_s": round(clone_tbs, 3), "required_bytes": need}
    for tag, key in (("hip", "match"), ("stats", "stats"), ("apply", "apply")):
        t = hip if tag == "hip" else med(s[tag])
        rate = need[key] / (t * 1e-3) / 1e12
        result[f"{key}_required_tb_per_s"] = round(rate, 3)
        result[f"{key}_fraction_of_clone_rate"] = round(rate / clone_tbs, 3)
    result["stats_ms"], result["fit_ms"], result["apply_ms"] = (round(med(s[k]), 4) for k in ("stats", "fit", "apply"))
    fb.emit("detailer_color_match", a, **result)


if __name__ == "__main__":
    main()
