#!/usr/bin/env python3
"""Multiband blend benchmark (lanpaint_amd.multiband on the HIP device): one JSON line.

Two cases at levels = 5, everything already on the device:

    frame  blend_multiband of 1 x 1024 x 1024 x 3 through a soft disc
    clip   the same for 81 x 720 x 1280 x 3, the disc drifting across the frame

    hip    lanpaint_amd.multiband: lp_multiband_blend (five reduce and five collapse launches)
    torch  the same rule restated in torch operators on the same device: REDUCE as two replicate-padded strided depthwise
           conv2d (rows, then columns), EXPAND as slices of the replicate-padded coarse level interleaved, the collapse level
           by level.  The values agree to rounding (conv2d fixes no order of its sums); the difference is printed.
    clone  torch.clone of the case's image: the copy rate this process reaches on these very tensors, in the same run.

    python scripts/bench_multiband.py [--iters 20] [--warmup 3]
    python scripts/bench_multiband.py --job hip --case frame --iters 10     # the body of a rocprofv3 --kernel-trace run

Time: featurebench.events per call; every iteration runs hip, torch, hip, torch, clone.  Bytes: what the rule has to move -- image1, image2
and the mask read twice (to build the pyramid and to collapse onto level 0: level 0 is never stored), the result written once,
and every stored level written once and read where the rule needs it -- over the time, and that rate over the clone's (one
read, one write).
"""
from __future__ import annotations

import featurebench as fb

CASES = {"frame": (1, 1024, 1024, 3), "clip": (81, 720, 1280, 3)}
LEVELS, RADIUS = 5, 150
K5 = (0.0625, 0.25, 0.375, 0.25, 0.0625)


def make_job(case, dev):
    import torch
    B, H, W, C = CASES[case]
    g = torch.Generator(device="cpu").manual_seed(0)
    a = (0.05 + 0.95 * torch.rand(B, H, W, C, generator=g)).to(dev)
    b = (0.05 + 0.95 * torch.rand(B, H, W, C, generator=g)).to(dev)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    mask = torch.zeros(B, H, W)
    for f in range(B):
        cx = W // 2 if B == 1 else 300 + (W - 600) * f // (B - 1)
        dist = ((yy - H // 2) ** 2 + (xx - cx) ** 2).float().sqrt()
        mask[f] = ((RADIUS - dist) / 8.0 + 0.5).clamp(0.0, 1.0)          # a disc with a soft rim of 8 pixels
    return {"case": case, "a": a, "b": b, "mask": mask.to(dev)}


def required_bytes(case):
    from lanpaint_amd import _cabi
    B, H, W, C = CASES[case]
    image, mask = B * H * W * C * 4, B * H * W * 4
    sizes = _cabi.multiband_levels(H, W, LEVELS)
    n = len(sizes) - 1
    pyramid = 0
    for l in range(1, n + 1):
        inner = l < n
        # D: written, read by the next REDUCE, by the collapse as the coarser level and as the finer one; W: written, read by the
        # next REDUCE and once by a collapse; R: written and read once (R_n is formed where it is read)
        pyramid += B * sizes[l][0] * sizes[l][1] * 4 * (C * (2 + 2 * inner) + (2 + inner) + C * 2 * inner)
    return {"job": 2 * (2 * image + mask) + image + pyramid, "pyramid": pyramid, "clone": 2 * image}


def hip_job(j):
    from lanpaint_amd import multiband
    return multiband.blend_multiband(j["a"], j["b"], j["mask"], LEVELS)


def clone(j):
    return j["a"].clone()


def _reduce(x):
    """[N, C, h, w] -> [N, C, ceil(h / 2), ceil(w / 2)]: rows, then columns."""
    import torch
    import torch.nn.functional as F
    c = x.shape[1]
    k = torch.tensor(K5, dtype=x.dtype, device=x.device)
    x = F.conv2d(F.pad(x, (0, 0, 2, 2), mode="replicate"), k.view(1, 1, 5, 1).expand(c, 1, 5, 1), stride=(2, 1), groups=c)
    return F.conv2d(F.pad(x, (2, 2, 0, 0), mode="replicate"), k.view(1, 1, 1, 5).expand(c, 1, 1, 5), stride=(1, 2), groups=c)


def _expand_axis(c, n, axis):
    import torch
    import torch.nn.functional as F
    pad = (0, 0, 1, 1) if axis == 2 else (1, 1, 0, 0)
    p = F.pad(c, pad, mode="replicate")
    m = c.shape[axis]
    lo, mid, hi = p.narrow(axis, 0, m), p.narrow(axis, 1, m), p.narrow(axis, 2, m)
    even = 0.125 * lo + 0.75 * mid + 0.125 * hi
    odd = 0.5 * mid + 0.5 * hi
    both = torch.stack((even, odd), dim=axis + 1)
    shape = list(c.shape)
    shape[axis] = 2 * m
    return both.reshape(shape).narrow(axis, 0, n)


def _expand(c, h, w):
    return _expand_axis(_expand_axis(c, h, 2), w, 3)


def torch_blend(a, b, mask, levels):
    """The rule of lanpaint_amd/multiband.py in torch operators: images [B, H, W, C], mask [Bm, H, W]."""
    import torch
    an = a.permute(0, 3, 1, 2)
    D = [b.permute(0, 3, 1, 2) - an]
    Wt = [torch.where(mask > 0, mask.clamp(max=1.0), 0.0).unsqueeze(1)]
    while len(D) <= levels and tuple(D[-1].shape[2:]) != (1, 1):
        D.append(_reduce(D[-1]))
        Wt.append(_reduce(Wt[-1]))
    R = Wt[-1] * D[-1]
    for l in range(len(D) - 2, -1, -1):
        h, w = D[l].shape[2:]
        R = _expand(R, h, w) + Wt[l] * (D[l] - _expand(D[l + 1], h, w))
    return (an + R).permute(0, 2, 3, 1).contiguous()


def torch_job(j):
    return torch_blend(j["a"], j["b"], j["mask"], LEVELS)


def run(job, iters, warmup, only=None):
    hip, eager, copy = (lambda f=f: f(job) for f in (hip_job, torch_job, clone))
    fns = [("hip_a", hip), ("torch_a", eager), ("hip_b", hip), ("torch_b", eager), ("clone", copy)]
    if only:
        fns = [(only + "_a", hip if only == "hip" else eager)]
    return fb.series(fns, iters, warmup)


def measure(case, dev, iters, warmup):
    import torch
    job = make_job(case, dev)
    diff = float((hip_job(job) - torch_job(job)).abs().max())       # the two sides compute the same thing
    torch.cuda.empty_cache()
    s = run(job, iters, warmup)
    med = fb.median
    need = required_bytes(case)
    hip, eager = med(s["hip_a"] + s["hip_b"]), med(s["torch_a"] + s["torch_b"])
    clone_tbs = need["clone"] / (med(s["clone"]) * 1e-3) / 1e12
    rate = need["job"] / (hip * 1e-3) / 1e12
    return {"case": case, "image": list(job["a"].shape), "levels": LEVELS, "max_abs_hip_minus_torch": diff,
            "hip_ms": round(hip, 4), "torch_ms": round(eager, 4), "torch_over_hip": round(eager / hip, 2),
            "hip_min_max_ms": fb.summary(s["hip_a"] + s["hip_b"])[1],
            "torch_min_max_ms": fb.summary(s["torch_a"] + s["torch_b"])[1],
            "hip_spread": fb.spread(s["hip_a"], s["hip_b"]),
            "torch_spread": fb.spread(s["torch_a"], s["torch_b"]),
            "clone_ms": round(med(s["clone"]), 4), "clone_tb_per_s": round(clone_tbs, 3), "required_bytes": need,
            "required_tb_per_s": round(rate, 3), "fraction_of_clone_rate": round(rate / clone_tbs, 3)}


def main():
    a = fb.parser(CASES, ("hip", "torch"), iters=20, warmup=3).parse_args()
    dev = fb.device()
    import torch
    cases = (a.case,) if a.case else tuple(CASES)
    if a.job:
        for case in cases:
            run(make_job(case, dev), a.iters, a.warmup, only=a.job)
        return
    results = []
    for case in cases:
        results.append(measure(case, dev, a.iters, a.warmup))
        torch.cuda.empty_cache()
    fb.emit("multiband_blend", a, results, hip_faster_in_every_case=all(r["torch_over_hip"] > 1.0 for r in results))


if __name__ == "__main__":
    main()
