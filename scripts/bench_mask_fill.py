#!/usr/bin/env python3
"""Masked-area fill and outpaint canvas benchmark (lanpaint_amd.fill on the HIP device): one JSON line.

Three cases, everything already on the device:

    frame     fill_masked of 1 x 720 x 1280 x 3 under a disc of radius 150
    clip      the same for 81 frames, the disc drifting across the frame
    outpaint  outpaint_pad of 81 x 480 x 480 x 3 to 480 x 880 (200 columns each side, the reference README's 1:1 -> 11:6),
              overlap 16, filled

    hip    lanpaint_amd.fill: lp_mask_fill (three launches each way at 720 x 1280), lp_outpaint_pad
    eager  the same rule composed from torch operators on the same device, level by level: masked sums of the four children
           in the rule's order and a division for the pull, gathers of the clamped taps and unfused products and sums for
           the push (the tap tables are built once and kept).  The yardstick: no earlier revision has a fill to time.
    clone  torch.clone of the case's image: the copy rate this process reaches on these very tensors, in the same run.

    python scripts/bench_mask_fill.py [--iters 20] [--warmup 3]
    python scripts/bench_mask_fill.py --job hip --case frame --iters 10     # the body of a rocprofv3 --kernel-trace run

Time: featurebench.events per call; every iteration runs hip, eager, hip, eager, clone.  Bytes: what the job has to move -- image and
mask read once, the result written once -- over the time, and that rate over the clone's (one read, one write).
"""
from __future__ import annotations

import featurebench as fb

CASES = ("frame", "clip", "outpaint")
H, W, C, FRAMES, RADIUS = 720, 1280, 3, 81, 150
OUT_SIDE, OUT_PAD, OVERLAP = 480, 200, 16
_TAPS = {}


def make_job(case, dev):
    import torch
    g = torch.Generator(device="cpu").manual_seed(0)
    if case == "outpaint":
        return {"case": case, "image": (0.05 + 0.95 * torch.rand(FRAMES, OUT_SIDE, OUT_SIDE, C, generator=g)).to(dev)}
    frames = 1 if case == "frame" else FRAMES
    image = (0.05 + 0.95 * torch.rand(frames, H, W, C, generator=g)).to(dev)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    mask = torch.zeros(frames, H, W)
    for f in range(frames):
        cx = W // 2 if frames == 1 else 300 + (W - 600) * f // (frames - 1)
        mask[f] = ((yy - H // 2) ** 2 + (xx - cx) ** 2 < RADIUS * RADIUS).float()
    return {"case": case, "image": image, "mask": mask.to(dev)}


def required_bytes(case):
    if case == "outpaint":
        src = FRAMES * OUT_SIDE * OUT_SIDE * C * 4
        canvas, mask = FRAMES * OUT_SIDE * (OUT_SIDE + 2 * OUT_PAD) * C * 4, OUT_SIDE * (OUT_SIDE + 2 * OUT_PAD) * 4
        return {"job": src + canvas + mask, "clone": 2 * src}       # the original read, the filled canvas and its mask written
    frames = 1 if case == "frame" else FRAMES
    image, mask = frames * H * W * C * 4, frames * H * W * 4
    return {"job": 2 * image + mask, "clone": 2 * image}


def hip_job(j):
    from lanpaint_amd import fill
    if j["case"] == "outpaint":
        return fill.outpaint_pad(j["image"], None, left=OUT_PAD, right=OUT_PAD, overlap=OVERLAP, multiple_of=8, fill=True)[0]
    return fill.fill_masked(j["image"], j["mask"])


def clone(j):
    return j["image"].clone()


def _taps(n_fine, n_coarse, dev):
    import torch
    key = (n_fine, n_coarse, str(dev))
    if key not in _TAPS:
        i = torch.arange(n_fine, device=dev)
        odd = (i % 2) == 1
        i0 = torch.where(odd, (i - 1) // 2, i // 2 - 1)
        a0 = torch.where(odd, 0.75, 0.25).float()
        _TAPS[key] = (i0.clamp(0, n_coarse - 1), (i0 + 1).clamp(0, n_coarse - 1), a0, 1.0 - a0)
    return _TAPS[key]


def eager_fill(image, mask):
    """The rule of lanpaint_amd/fill.py in torch operators: image [B, H, W, C], mask [Bm, H, W]."""
    import torch
    import torch.nn.functional as F
    known = ~(mask > 0.5)
    if known.shape[0] != image.shape[0]:
        known = known.expand(image.shape[0], -1, -1)
    v, k = [torch.where(known[..., None], image, 0.0)], [known]
    while tuple(v[-1].shape[1:3]) != (1, 1):
        h, w = v[-1].shape[1:3]
        vp = F.pad(v[-1], (0, 0, 0, w % 2, 0, h % 2))
        kp = F.pad(k[-1].float(), (0, w % 2, 0, h % 2)) > 0
        s = torch.zeros_like(vp[:, ::2, ::2])
        n = torch.zeros_like(kp[:, ::2, ::2], dtype=torch.float32)
        for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
            present = kp[:, dy::2, dx::2]
            s = torch.where(present[..., None], s + vp[:, dy::2, dx::2], s)
            n = n + present
        v.append(torch.where((n > 0)[..., None], s / n[..., None], 0.0))
        k.append(n > 0)
    f = v[-1]
    for l in range(len(v) - 2, -1, -1):
        h, w = v[l].shape[1:3]
        ty0, ty1, a0, a1 = _taps(h, f.shape[1], f.device)
        tx0, tx1, b0, b1 = _taps(w, f.shape[2], f.device)
        r = a0[None, :, None, None] * f[:, ty0] + a1[None, :, None, None] * f[:, ty1]
        up = b0[None, None, :, None] * r[:, :, tx0] + b1[None, None, :, None] * r[:, :, tx1]
        f = torch.where(k[l][..., None], v[l], up)
    return torch.where(k[-1].reshape(-1, 1, 1, 1), torch.where(known[..., None], image, f), image)


def eager_job(j):
    import torch
    import torch.nn.functional as F
    if j["case"] != "outpaint":
        return eager_fill(j["image"], j["mask"])
    canvas = F.pad(j["image"], (0, 0, OUT_PAD, OUT_PAD))
    mask = torch.ones(1, OUT_SIDE, OUT_SIDE + 2 * OUT_PAD, device=canvas.device)
    mask[:, :, OUT_PAD + OVERLAP: OUT_PAD + OUT_SIDE - OVERLAP] = 0.0
    return eager_fill(canvas, mask)


def run(job, iters, warmup, only=None):
    hip, eager, copy = (lambda f=f: f(job) for f in (hip_job, eager_job, clone))
    fns = [("hip_a", hip), ("eager_a", eager), ("hip_b", hip), ("eager_b", eager), ("clone", copy)]
    if only:
        fns = [(only + "_a", hip if only == "hip" else eager)]
    return fb.series(fns, iters, warmup)


def measure(case, dev, iters, warmup):
    job = make_job(case, dev)
    diff = float((hip_job(job) - eager_job(job)).abs().max())       # the two sides compute the same thing
    s = run(job, iters, warmup)
    med = fb.median
    need = required_bytes(case)
    hip, eager = med(s["hip_a"] + s["hip_b"]), med(s["eager_a"] + s["eager_b"])
    clone_tbs = need["clone"] / (med(s["clone"]) * 1e-3) / 1e12
    rate = need["job"] / (hip * 1e-3) / 1e12
    return {"case": case, "image": list(job["image"].shape), "max_abs_hip_minus_eager": diff,
            "hip_ms": round(hip, 4), "eager_ms": round(eager, 4), "eager_over_hip": round(eager / hip, 2),
            "hip_min_max_ms": fb.summary(s["hip_a"] + s["hip_b"])[1],
            "eager_min_max_ms": fb.summary(s["eager_a"] + s["eager_b"])[1],
            "hip_spread": fb.spread(s["hip_a"], s["hip_b"]),
            "eager_spread": fb.spread(s["eager_a"], s["eager_b"]),
            "clone_ms": round(med(s["clone"]), 4), "clone_tb_per_s": round(clone_tbs, 3), "required_bytes": need,
            "required_tb_per_s": round(rate, 3), "fraction_of_clone_rate": round(rate / clone_tbs, 3)}


def main():
    a = fb.parser(CASES, ("hip", "eager"), iters=20, warmup=3).parse_args()
    dev = fb.device()
    import torch
    cases = (a.case,) if a.case else CASES
    if a.job:
        for case in cases:
            run(make_job(case, dev), a.iters, a.warmup, only=a.job)
        return
    results = []
    for case in cases:
        results.append(measure(case, dev, a.iters, a.warmup))
        torch.cuda.empty_cache()
    fb.emit("mask_fill", a, results, hip_faster_in_every_case=all(r["eager_over_hip"] > 1.0 for r in results))


if __name__ == "__main__":
    main()
