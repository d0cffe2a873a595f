#!/usr/bin/env python3
"""Detailer crop / stitch benchmark (lanpaint_amd.detail on the HIP device) against what the package could do for the same
job without it: one JSON line.

Shapes (image, mask and detailed crop already on the device):
    still  1 x 2160 x 3840 x 3, mask box 400 x 560 -> region 504 x 704 (context 1.25), worked at 1024 long side
    clip   81 x 720 x 1280 x 3, mask box 288 x 384 -> region 360 x 480 (context 1.25), worked at 768 long side

Jobs:
    crop    detail.crop_resample(image, mask)            vs  slicing + F.interpolate(antialias=True) of image and mask
    stitch  detail.stitch(original, detail, mask, k=9)   vs  clone + slice-assign of the interpolated detail +
                                                             blend.merge_video_with_mask over the full frame

    python scripts/bench_detailer.py [--iters 30] [--warmup 5] [--filter bicubic] [--kernels still:crop=A.db clip:stitch=B.db]
    python scripts/bench_detailer.py --shape clip --job stitch --iters 5   # the body of a rocprofv3 --kernel-trace run (new path only)

Time: featurebench.events per call; every iteration runs new, old, new, old.  Per-kernel times come from a SEPARATE
rocprofv3 --kernel-trace --stats run per shape and job (--kernels reads its results .db / kernel-trace CSV); required bytes over
kernel time are reported against 6.29 TB/s achievable copy rate.
"""
from __future__ import annotations

import featurebench as fb

COPY_ACHIEVABLE = 6.29e12
# name: (B, H, W, C, mask box (y0, y1, x0, x1) inclusive, context, target)
SHAPES = {"still": (1, 2160, 3840, 3, (900, 1299, 1600, 2159), 1.25, 1024),
          "clip": (81, 720, 1280, 3, (200, 487, 400, 783), 1.25, 768)}
K = 9
KERNELS = ("bbox", "resample", "crop", "copy", "stitch")


def make_job(name, filter, dev):
    import torch
    from lanpaint_amd import detail
    b, H, W, c, (y0, y1, x0, x1), context, target = SHAPES[name]
    g = torch.Generator(device="cpu").manual_seed(0)
    image = torch.rand(b, H, W, c, generator=g).to(dev)
    mask = torch.zeros(1, H, W)
    mask[0, y0:y1 + 1, x0:x1 + 1] = 1.0
    mask = mask.to(dev)
    region = detail.plan_region(detail.mask_bbox(mask), H, W, context, 0, 8, target)
    det = torch.rand(b, region.oh, region.ow, c, generator=g).to(dev)
    return image, mask, region, det


def crop_new(image, mask, r, det, filter):
    from lanpaint_amd import detail
    return detail.crop_resample(image, mask, r, filter)


def crop_old(image, mask, r, det, filter):
    import torch.nn.functional as F
    win = image[:, r.y0:r.y0 + r.h, r.x0:r.x0 + r.w, :].movedim(-1, 1)
    img = F.interpolate(win, size=(r.oh, r.ow), mode=filter, align_corners=False, antialias=True).movedim(1, -1).contiguous()
    m = F.interpolate(mask[:, None, r.y0:r.y0 + r.h, r.x0:r.x0 + r.w], size=(r.oh, r.ow), mode="bilinear",
                      align_corners=False, antialias=True)[:, 0]
    return img, m


def stitch_new(image, mask, r, det, filter):
    from lanpaint_amd import detail
    return detail.stitch(image, det, mask, r, K, filter)


def stitch_old(image, mask, r, det, filter):
    import torch.nn.functional as F
    from lanpaint_amd import blend
    back = F.interpolate(det.movedim(-1, 1), size=(r.h, r.w), mode=filter, align_corners=False, antialias=True).movedim(1, -1)
    pasted = image.clone()
    pasted[:, r.y0:r.y0 + r.h, r.x0:r.x0 + r.w, :] = back
    return blend.merge_video_with_mask(image, pasted, mask, K)


JOBS = {"crop": (crop_new, crop_old), "stitch": (stitch_new, stitch_old)}


def required_bytes(name, job, r):
    b, H, W, c = SHAPES[name][:4]
    if job == "crop":                                     # window in + working size out, image and the one-frame mask
        return 4 * (b * c + 1) * (r.h * r.w + r.oh * r.ow)
    halo = (r.h + 2 * (K - 1)) * (r.w + 2 * (K - 1))      # stitch: frame in + frame out + window terms
    return 4 * (2 * b * H * W * c + b * c * (r.oh * r.ow + 4 * r.h * r.w) + b * halo)


def run_shape(name, iters, warmup, filter, new_only=False, only=None):
    args = make_job(name, filter, fb.device()) + (filter,)
    series = {}
    for job, (new, old) in JOBS.items():
        if only and job != only:
            continue
        new, old = (lambda f=f: f(*args) for f in (new, old))
        fns = [("new_a", new), ("new_b", new)] if new_only else [("new_a", new), ("old_a", old), ("new_b", new), ("old_b", old)]
        series[job] = fb.series(fns, iters, warmup)
    return args[2], series


def kernel_stats(path, job):
    """Per detail kernel of a trace that ran ONE job: calls, total and median time; and the kernel time of one call of the job
    (a crop is two resample launches, image and mask; a stitch is one stitch launch plus its resample-back and copy)."""
    from rocprof_summary import rows_from_csv, rows_from_db
    rows = rows_from_db(path) if path.endswith(".db") else rows_from_csv(path)
    per = {}
    for name, start, end, *_ in rows:
        for k in KERNELS:
            if f"lp_detail_{k}_kernel" in name:
                per.setdefault(k, []).append((end - start) * 1e-3)
    out = {k: {"calls": len(v), "total_us": round(sum(v), 2), "median_us": round(fb.median(v), 2)} for k, v in per.items()}
    anchor = "stitch" if job == "stitch" else "resample"
    if anchor not in per:
        return out, None
    calls = len(per[anchor]) / (1 if job == "stitch" else 2)
    return out, sum(sum(v) for k, v in per.items() if k != "bbox") / calls


def main():
    ap = fb.parser(iters=30, warmup=5)
    ap.add_argument("--filter", choices=("bilinear", "bicubic"), default="bicubic")
    ap.add_argument("--shape", choices=sorted(SHAPES))
    ap.add_argument("--job", choices=sorted(JOBS), help="with --shape: run this job only")
    ap.add_argument("--kernels", nargs="*", default=[], help="SHAPE:JOB=rocprofv3 results .db or kernel-trace .csv")
    a = ap.parse_args()
    fb.device()
    import torch
    if a.shape:
        run_shape(a.shape, a.iters, a.warmup, a.filter, new_only=True, only=a.job)
        return
    profiles = dict(kv.split("=", 1) for kv in a.kernels)
    shapes = {}
    med = fb.median
    for name in sorted(SHAPES):
        region, series = run_shape(name, a.iters, a.warmup, a.filter)
        rec = {"image": list(SHAPES[name][:4]), "region": [region.y0, region.x0, region.h, region.w],
               "working_size": [region.oh, region.ow]}
        for job, s in series.items():
            new, old = med(s["new_a"] + s["new_b"]), med(s["old_a"] + s["old_b"])
            rec[job] = {"new_ms": round(new, 4), "old_ms": round(old, 4), "old_over_new": round(old / new, 3),
                        "new_min_max_ms": fb.summary(s["new_a"] + s["new_b"])[1],
                        "old_min_max_ms": fb.summary(s["old_a"] + s["old_b"])[1],
                        "spread_new": fb.spread(s["new_a"], s["new_b"]),
                        "spread_old": fb.spread(s["old_a"], s["old_b"]),
                        "required_bytes": required_bytes(name, job, region)}
        for job in JOBS:
            if f"{name}:{job}" in profiles:
                ks, per_call_us = kernel_stats(profiles[f"{name}:{job}"], job)
                rec[job]["kernels"] = ks
                if per_call_us:
                    rec[job]["kernel_us_per_call"] = round(per_call_us, 2)
                    rec[job]["copy_rate_frac"] = round(rec[job]["required_bytes"] / (per_call_us * 1e-6) / COPY_ACHIEVABLE, 4)
            else:
                rec[job]["kernels"] = "not measured"
        shapes[name] = rec
        torch.cuda.empty_cache()
    fb.emit("detailer_crop_stitch", a, filter=a.filter, blend_overlap=K, shapes=shapes)


if __name__ == "__main__":
    main()
