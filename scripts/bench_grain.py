#!/usr/bin/env python3
"""Grain match benchmark (lanpaint_amd.grain on the HIP device): one JSON line.

Two workloads, everything already on the device: a ramp with a 3 x 3 binomial grain of 0.03, clean under a box mask.

    still   1 image of 1024 x 1024 x 3
    clip    81 frames of 1280 x 720 x 3

    stats_out  grain.grain_stats(image, mask, "outside"): the reference side's measurement, one launch and its memset
    stats_in   grain.grain_stats(image, mask, "inside"): the generated side's
    fit        grain.grain_fit on the two tables: one small launch
    apply      grain.grain_apply with the fit's tables: one launch
    match      grain.match: the four together
    torch      the rule of the two heavy launches in torch operators on the same device: stats "inside" (the codes, max / min
               pooling, three separable filters as shifted slices, eight masked sums) and apply (Philox4x32-10 in int64 arithmetic, the size's
               filter, the tone-band interpolation).  Its results are compared with the launches'; the counts of differing
               elements are printed.
    clone      torch.clone of the image: 4 bytes read and 4 written per element.  apply has to move those and the mask
               (B * H * W * (8 C + 4) bytes); a stats launch reads image and mask once (B * H * W * (4 C + 4)).

    python scripts/bench_grain.py [--iters 10] [--warmup 2] [--case still] [--torch-iters 3]
    python scripts/bench_grain.py --job apply --case clip --iters 10      # the body of a rocprofv3 --kernel-trace run

Time: featurebench.events per call; every iteration runs apply, stats_in, apply, stats_in, stats_out, fit, clone, match.
"""
from __future__ import annotations

import featurebench as fb

CASES = {"still": (1, 1024, 1024, 3), "clip": (81, 720, 1280, 3)}
INFINITY_CACHE_BYTES = 256 << 20
SEED = 7
K = 8
M32 = 0xFFFFFFFF


def make_job(case, dev):
    import torch
    from lanpaint_amd import grain
    B, H, W, C = CASES[case]
    g = torch.Generator(device=dev).manual_seed(0)
    n = torch.randn(B, C, H + 2, W + 2, device=dev, generator=g)
    k = torch.tensor([[1., 2., 1.], [2., 4., 2.], [1., 2., 1.]], device=dev).div(6.0).view(1, 1, 3, 3).repeat(C, 1, 1, 1)
    noise = torch.nn.functional.conv2d(n, k, groups=C).permute(0, 2, 3, 1)
    del n
    ramp = torch.linspace(0.2, 0.8, W, device=dev).view(1, 1, W, 1)
    mask = torch.zeros(B, H, W, device=dev)
    mask[:, H // 4:3 * H // 4, W // 4:3 * W // 4] = 1.0
    image = (ramp + 0.03 * noise * (1.0 - mask[..., None])).contiguous()
    del noise
    job = {"case": case, "image": image, "mask": mask}
    job["out_t"] = grain.grain_stats(image, mask, "outside")
    job["in_t"] = grain.grain_stats(image, mask, "inside")
    job["amp"], job["size"] = grain.grain_fit(job["in_t"], job["out_t"])
    return job


# ---- the rule in torch operators --------------------------------------------------------------------------------------------
def torch_codes(x):
    import torch
    t = torch.where(x > 0, torch.clamp(x, max=1.0), torch.zeros_like(x))
    return (t * 255.0 + 0.5).to(torch.int32)


def _conv(q, taps):
    """sum t(dy) t(dx) q(y + dy, x + dx) over q [B, C, H, W] fp32 holding integers, for the separable kernel t x t: shifted slices
    along x, then along y (every partial sum is an integer below 2^24: exact, whatever the order)."""
    n = len(taps)
    w = q.shape[3] - n + 1
    row = sum(t * q[:, :, :, i:i + w] for i, t in enumerate(taps) if t)
    h = q.shape[2] - n + 1
    return sum(t * row[:, :, i:i + h] for i, t in enumerate(taps) if t)


B3, N3, N5, BIN5 = (1, 2, 1), (1, -2, 1), (1, 0, -2, 0, 1), (1, 4, 6, 4, 1)     # the 1-D taps of the separable kernels


def torch_stats_inside(image, mask, flat=64):
    import torch
    F = torch.nn.functional
    q = torch_codes(image).permute(0, 3, 1, 2).float()
    hi, lo = F.max_pool2d(q, 5, 1), -F.max_pool2d(-q, 5, 1)
    inside = -F.max_pool2d(-(mask > 0.5).float().unsqueeze(1), 5, 1) > 0
    take = inside & (hi - lo <= flat)
    mu16, e1, e2 = _conv(q[:, :, 1:-1, 1:-1], B3), _conv(q[:, :, 1:-1, 1:-1], N3), _conv(q, N5)
    band = (mu16.to(torch.int64) * K) // 4081
    e1, e2 = e1.to(torch.int64) ** 2, e2.to(torch.int64) ** 2
    rows = []
    for k in range(K):
        sel = take & (band == k)
        rows.append(torch.stack([sel.sum((2, 3)), (e1 * sel).sum((2, 3)), (e2 * sel).sum((2, 3))], dim=-1))
    return torch.stack(rows, dim=2)


def _mulhilo(m, c):
    """The high and low words of m * c, m a 32-bit constant, c int64 holding 32-bit words: products of 32 x 16 bits."""
    a, b = m * (c & 0xFFFF), m * (c >> 16)
    return (b + (a >> 16)) >> 16, (a + ((b & 0xFFFF) << 16)) & M32


def torch_philox(ctr, subseq, seed):
    c0, c1, c2, c3 = ctr & M32, ctr >> 32, torch_full(ctr, subseq & M32), torch_full(ctr, subseq >> 32)
    k0, k1 = seed & M32, seed >> 32
    for _ in range(10):
        hi0, lo0 = _mulhilo(0xD2511F53, c0)
        hi1, lo1 = _mulhilo(0xCD9E8D57, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def torch_full(like, value):
    import torch
    return torch.full_like(like, value)


def torch_field(B, H, W, C, sizes, seed, dev, frame0=0):
    """The integer grain as fp32 [B, H, W, C]; sizes: a list, one per image."""
    import torch
    yy, xx = torch.meshgrid(torch.arange(H + 4, device=dev), torch.arange(W + 4, device=dev), indexing="ij")
    ctr = yy * (W + 4) + xx
    out = torch.empty(B, H, W, C, device=dev)
    kernels = ((1,), B3, BIN5)
    for i in range(B):
        w = []
        for g in range((C + 3) // 4):
            words = torch_philox(ctr, (frame0 + i) * 16 + g, seed)
            for j in range(min(4, C - 4 * g)):
                v = words[j]
                w.append((v & 255) + ((v >> 8) & 255) + ((v >> 16) & 255) + (v >> 24) - 510)
        w = torch.stack(w).float().unsqueeze(0)
        s = sizes[i]
        out[i] = _conv(w[:, :, 2 - s:H + 2 + s, 2 - s:W + 2 + s], kernels[s])[0].permute(1, 2, 0)
    return out


def torch_apply(image, mask, amp, sizes, seed):
    import torch
    B, H, W, C = image.shape
    g = torch_field(B, H, W, C, sizes, seed, image.device)
    q = torch.nn.functional.pad(torch_codes(image).permute(0, 3, 1, 2).float(), (1, 1, 1, 1), mode="replicate")
    mu16 = _conv(q, B3).permute(0, 2, 3, 1)
    # the quotient through fp64: correctly rounded to fp32 (53 >= 2 * 24 + 2), which torch's own fp32 division on the device is not
    u = (((mu16 * K).double() / 4080.0).float() - 0.5).clamp(0.0, K - 1.0)
    k0 = u.to(torch.int64).clamp(max=K - 2)
    f = u - k0.float()
    table = amp.view(B, 1, 1, C, K).expand(B, H, W, C, K)
    a0, a1 = table.gather(4, k0.unsqueeze(-1)).squeeze(-1), table.gather(4, (k0 + 1).unsqueeze(-1)).squeeze(-1)
    a = a0 + f * (a1 - a0)
    m = torch.where(mask > 0, torch.clamp(mask, max=1.0), torch.zeros_like(mask)).unsqueeze(-1)
    t = m * a
    return torch.where(t == 0, image, image + t * g)


# ---- timing -----------------------------------------------------------------------------------------------------------------
def jobs():
    from lanpaint_amd import grain
    return {"stats_out": lambda j: grain.grain_stats(j["image"], j["mask"], "outside"),
            "stats_in": lambda j: grain.grain_stats(j["image"], j["mask"], "inside"),
            "fit": lambda j: grain.grain_fit(j["in_t"], j["out_t"]),
            "apply": lambda j: grain.grain_apply(j["image"], j["mask"], j["amp"], j["size"], SEED),
            "match": lambda j: grain.match(j["image"], j["mask"], seed=SEED),
            "clone": lambda j: j["image"].clone(),
            "torch_stats": lambda j: torch_stats_inside(j["image"], j["mask"]),
            "torch_apply": lambda j: torch_apply(j["image"], j["mask"], j["amp"], j["sizes_host"], SEED)}


def run(job, order, iters, warmup):
    fn = {name: (lambda f=f: f(job)) for name, f in jobs().items()}
    return fb.series([(tag, fn[name]) for tag, name in order], iters, warmup)


def measure(job, iters, warmup, torch_iters):
    import torch
    fn = jobs()
    job["sizes_host"] = job["size"].tolist()                            # the torch form picks its kernel on the host
    B, H, W, C = CASES[job["case"]]
    stats_diff = int((fn["stats_in"](job) != torch_stats_inside(job["image"], job["mask"])).sum())
    got, eager = fn["apply"](job), fn["torch_apply"](job)
    apply_diff = int((got.view(torch.int32) != eager.view(torch.int32)).sum())
    changed = int((got != job["image"]).sum())
    del got, eager
    torch.cuda.empty_cache()
    s = run(job, [("apply_a", "apply"), ("stats_in_a", "stats_in"), ("apply_b", "apply"), ("stats_in_b", "stats_in"),
                  ("stats_out", "stats_out"), ("fit", "fit"), ("clone", "clone"), ("match", "match")], iters, warmup)
    t = run(job, [("torch_stats", "torch_stats"), ("torch_apply", "torch_apply")], torch_iters, 1)
    torch.cuda.empty_cache()
    med = fb.median
    apply, stats_in = med(s["apply_a"] + s["apply_b"]), med(s["stats_in_a"] + s["stats_in_b"])
    clone = med(s["clone"])
    apply_bytes, stats_bytes, clone_bytes = B * H * W * (8 * C + 4), B * H * W * (4 * C + 4), B * H * W * C * 8
    r3 = lambda v: round(v, 4)                                          # noqa: E731
    return {"case": job["case"], "shape": [B, H, W, C], "fitted_size": job["sizes_host"][0],
            "grain_std_codes_max": r3(float(job["amp"].max()) * 255.0 * (21845 * (1, 36, 4900)[job["sizes_host"][0]]) ** 0.5),
            "stats_elements_differing_from_torch": stats_diff, "apply_elements_differing_from_torch": apply_diff,
            "elements_changed_by_apply": changed,
            "match_ms": r3(med(s["match"])), "match_min_max_ms": fb.summary(s["match"])[1],
            "stats_out_ms": r3(med(s["stats_out"])), "stats_in_ms": r3(stats_in), "fit_ms": r3(med(s["fit"])), "apply_ms": r3(apply),
            "apply_min_max_ms": fb.summary(s["apply_a"] + s["apply_b"])[1],
            "stats_in_min_max_ms": fb.summary(s["stats_in_a"] + s["stats_in_b"])[1],
            "apply_spread": fb.spread(s["apply_a"], s["apply_b"]),
            "stats_in_spread": fb.spread(s["stats_in_a"], s["stats_in_b"]),
            "clone_ms": r3(clone), "torch_stats_ms": r3(med(t["torch_stats"])), "torch_apply_ms": r3(med(t["torch_apply"])),
            "torch_stats_over_stats_in": round(med(t["torch_stats"]) / stats_in, 1),
            "torch_apply_over_apply": round(med(t["torch_apply"]) / apply, 1),
            "apply_over_clone": round(apply / clone, 2), "stats_in_over_clone": round(stats_in / clone, 2),
            "apply_required_bytes": apply_bytes, "stats_required_bytes": stats_bytes,
            "apply_fits_infinity_cache": apply_bytes <= INFINITY_CACHE_BYTES,
            "apply_tb_per_s": round(apply_bytes / (apply * 1e-3) / 1e12, 3),
            "stats_in_tb_per_s": round(stats_bytes / (stats_in * 1e-3) / 1e12, 3),
            "clone_tb_per_s": round(clone_bytes / (clone * 1e-3) / 1e12, 3)}


def main():
    ap = fb.parser(CASES, ("stats_out", "stats_in", "fit", "apply", "match"))
    ap.add_argument("--torch-iters", type=int, default=3)
    a = ap.parse_args()
    dev = fb.device()
    import torch
    results = []
    for case in ((a.case,) if a.case else tuple(CASES)):
        job = make_job(case, dev)
        if a.job:
            run(job, [(a.job, a.job)], a.iters, a.warmup)
        else:
            results.append(measure(job, a.iters, a.warmup, a.torch_iters))
        del job
        torch.cuda.empty_cache()
    if not a.job:
        fb.emit("grain_match", a, results, torch_iters=a.torch_iters)


if __name__ == "__main__":
    main()
