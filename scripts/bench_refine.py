#!/usr/bin/env python3
"""Mask refine benchmark (lanpaint_amd.refine on the HIP device): one JSON line.

Two cases at radius 8 and 32 (and the HIP side alone at 64), eps = 1e-3, everything already on the device:

    frame  refine_mask of 1 x 1024 x 1024 x 3 through a rough disc
    clip   the same for 81 x 720 x 1280 x 3, the disc drifting across the frame

    hip    lanpaint_amd.refine: lp_mask_refine (two launches per chunk of the batch)
    torch  the same filter in torch operators on the same device, fp32: the thirteen box means through two cumsum passes and
           index_select differences, the 3 x 3 solve by the adjugate written out plane by plane, four more box means.  It
           fixes no order of its sums and works on [0, 1] values, not on 8-bit codes: the values agree to the codes' step
           (a few 1e-3), the difference is printed, and so is how many pixels each side leaves on the wrong side of the
           guide's disc.
    clone  torch.clone of the case's image: the copy rate this process reaches on these very tensors, in the same run.

    python scripts/bench_refine.py [--iters 10] [--warmup 2]
    python scripts/bench_refine.py --job hip --case frame --radius 8 --iters 10     # the body of a rocprofv3 --kernel-trace run

Time: featurebench.events per call; every iteration runs hip, torch, hip, torch, clone.  Bytes: what the rule has to move -- the guide and
the mask read, the result written, the 16 bytes per pixel of the workspace written once and read once -- over the time, and that
rate over the clone's (one read, one write).
"""
from __future__ import annotations

import featurebench as fb

CASES = {"frame": (1, 1024, 1024, 3), "clip": (81, 720, 1280, 3)}
RADII, HIP_ONLY_RADIUS = (8, 32), 64
EPS, DISC = 1e-3, 150


def make_job(case, dev):
    import torch
    B, H, W, C = CASES[case]
    g = torch.Generator(device="cpu").manual_seed(0)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    guide = torch.empty(B, H, W, C)
    mask = torch.empty(B, H, W)
    inside, outside = torch.tensor([0.8, 0.3, 0.2]), torch.tensor([0.2, 0.5, 0.7])
    for f in range(B):
        cx = W // 2 if B == 1 else 300 + (W - 600) * f // (B - 1)
        dist = ((yy - H // 2) ** 2 + (xx - cx) ** 2).float().sqrt()
        guide[f] = torch.where((dist < DISC).unsqueeze(-1), inside, outside)
        mask[f] = (dist + 3.0 * torch.sin(yy / 3.0) + 2.0 < DISC).float()          # the disc, ragged and 2 pixels short
    guide += 0.02 * torch.randn(B, H, W, C, generator=g)
    return {"case": case, "guide": guide.to(dev), "mask": mask.to(dev)}


def required_bytes(case):
    B, H, W, C = CASES[case]
    pix = B * H * W
    return {"job": pix * (4 * C + 4 + 4 + 2 * 16), "workspace": pix * 16, "clone": 2 * pix * C * 4}


def hip_job(j, r):
    from lanpaint_amd import refine
    return refine.refine_mask(j["guide"], j["mask"], r, EPS)


def clone(j, r):
    return j["guide"].clone()


def _box_mean(x, r):
    """[B, K, H, W] -> the mean over the (2r + 1) window cut at the border: two cumsum passes, differences by index_select."""
    import torch
    import torch.nn.functional as F
    H, W = x.shape[2:]
    dev = x.device
    c = F.pad(x.cumsum(2), (0, 0, 1, 0))
    y0, y1 = (torch.arange(H, device=dev) - r).clamp(0, H), (torch.arange(H, device=dev) + r + 1).clamp(0, H)
    x = c.index_select(2, y1) - c.index_select(2, y0)
    c = F.pad(x.cumsum(3), (1, 0, 0, 0))
    x0, x1 = (torch.arange(W, device=dev) - r).clamp(0, W), (torch.arange(W, device=dev) + r + 1).clamp(0, W)
    x = c.index_select(3, x1) - c.index_select(3, x0)
    n = ((y1 - y0).view(H, 1) * (x1 - x0).view(1, W)).to(x.dtype)
    return x / n


def torch_refine(guide, mask, r, eps):
    """The colour guided filter in torch operators: guide [B, H, W, C >= 3], mask [B, H, W] -> [B, H, W]."""
    import torch
    I = guide[..., :3].permute(0, 3, 1, 2).clamp(0.0, 1.0)
    p = mask.clamp(0.0, 1.0).unsqueeze(1)
    planes = torch.cat([I, p, I * p, I[:, 0:1] * I, I[:, 1:2] * I[:, 1:], I[:, 2:3] * I[:, 2:]], dim=1)       # 13
    m = _box_mean(planes, r)
    mI, mp = m[:, 0:3], m[:, 3:4]
    cov = m[:, 4:7] - mI * mp
    v00 = m[:, 7] - mI[:, 0] * mI[:, 0] + eps
    v01 = m[:, 8] - mI[:, 0] * mI[:, 1]
    v02 = m[:, 9] - mI[:, 0] * mI[:, 2]
    v11 = m[:, 10] - mI[:, 1] * mI[:, 1] + eps
    v12 = m[:, 11] - mI[:, 1] * mI[:, 2]
    v22 = m[:, 12] - mI[:, 2] * mI[:, 2] + eps
    c00, c01, c02 = v11 * v22 - v12 * v12, v02 * v12 - v01 * v22, v01 * v12 - v02 * v11
    c11, c12, c22 = v00 * v22 - v02 * v02, v01 * v02 - v00 * v12, v00 * v11 - v01 * v01
    det = v00 * c00 + v01 * c01 + v02 * c02
    a = torch.stack([c00 * cov[:, 0] + c01 * cov[:, 1] + c02 * cov[:, 2], c01 * cov[:, 0] + c11 * cov[:, 1] + c12 * cov[:, 2],
                     c02 * cov[:, 0] + c12 * cov[:, 1] + c22 * cov[:, 2]], dim=1) / det.unsqueeze(1)
    b = mp - (a * mI).sum(1, keepdim=True)
    q = _box_mean(torch.cat([a, b], dim=1), r)
    return ((q[:, 0:3] * I).sum(1) + q[:, 3]).clamp(0.0, 1.0)


def torch_job(j, r):
    return torch_refine(j["guide"], j["mask"], r, EPS)


def run(job, r, iters, warmup, only=None):
    hip, eager, copy = (lambda f=f: f(job, r) for f in (hip_job, torch_job, clone))
    fns = [("hip_a", hip), ("torch_a", eager), ("hip_b", hip), ("torch_b", eager), ("clone", copy)]
    if only:
        fns = [(only + "_a", hip if only == "hip" else eager)]
    return fb.series(fns, iters, warmup)


def measure(job, r, iters, warmup):
    import torch
    case = job["case"]
    got, eager = hip_job(job, r), torch_job(job, r)
    truth = job["guide"][..., 0] > 0.5                               # the disc the guide shows
    diff = float((got - eager).abs().max())
    wrong = {"rough": int(((job["mask"] > 0.5) != truth).sum()), "hip": int(((got > 0.5) != truth).sum()),
             "torch": int(((eager > 0.5) != truth).sum())}
    del got, eager, truth
    torch.cuda.empty_cache()
    s = run(job, r, iters, warmup)
    med = fb.median
    need = required_bytes(case)
    hip, eager = med(s["hip_a"] + s["hip_b"]), med(s["torch_a"] + s["torch_b"])
    clone_tbs = need["clone"] / (med(s["clone"]) * 1e-3) / 1e12
    rate = need["job"] / (hip * 1e-3) / 1e12
    return {"case": case, "image": list(job["guide"].shape), "radius": r, "eps": EPS, "max_abs_hip_minus_torch": diff,
            "pixels_on_the_wrong_side": wrong,
            "hip_ms": round(hip, 4), "torch_ms": round(eager, 4), "torch_over_hip": round(eager / hip, 2),
            "hip_min_max_ms": fb.summary(s["hip_a"] + s["hip_b"])[1],
            "torch_min_max_ms": fb.summary(s["torch_a"] + s["torch_b"])[1],
            "hip_spread": fb.spread(s["hip_a"], s["hip_b"]),
            "torch_spread": fb.spread(s["torch_a"], s["torch_b"]),
            "clone_ms": round(med(s["clone"]), 4), "clone_tb_per_s": round(clone_tbs, 3), "required_bytes": need,
            "required_tb_per_s": round(rate, 3), "fraction_of_clone_rate": round(rate / clone_tbs, 3)}


def measure_hip_only(job, r, iters, warmup):
    ms, low_high = fb.summary(run(job, r, iters, warmup, only="hip")["hip_a"])
    return {"case": job["case"], "radius": r, "hip_ms": ms, "hip_min_max_ms": low_high}


def main():
    ap = fb.parser(CASES, ("hip", "torch"))
    ap.add_argument("--radius", type=int, help="this radius only")
    a = ap.parse_args()
    dev = fb.device()
    import torch
    cases = (a.case,) if a.case else tuple(CASES)
    radii = (a.radius,) if a.radius else RADII
    if a.job:
        for case in cases:
            job = make_job(case, dev)
            for r in radii:
                run(job, r, a.iters, a.warmup, only=a.job)
        return
    results, largest = [], []
    for case in cases:
        job = make_job(case, dev)
        for r in radii:
            results.append(measure(job, r, a.iters, a.warmup))
            torch.cuda.empty_cache()
        if not a.radius:
            largest.append(measure_hip_only(job, HIP_ONLY_RADIUS, a.iters, a.warmup))
        del job
        torch.cuda.empty_cache()
    fb.emit("mask_refine", a, results, radius_64_hip_only=largest, hip_faster_in_every_case=all(r["torch_over_hip"] > 1.0 for r in results))


if __name__ == "__main__":
    main()
