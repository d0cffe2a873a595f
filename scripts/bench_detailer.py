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

Time: device events around one call, per iteration.  Every iteration runs new, old, new, old: the two series of the SAME code
give the spread (relative difference of their medians), which is what a new-vs-old difference has to exceed to mean
anything.  Per-kernel times come from a SEPARATE rocprofv3 --kernel-trace --stats run per shape and job (--kernels reads its
results .db / kernel-trace CSV); required bytes over kernel time are reported against 6.29 TB/s achievable copy rate.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

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


def timed(fn, args):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn(*args)
    e1.record()
    e1.synchronize()
    del out
    return e0.elapsed_time(e1)


def required_bytes(name, job, r):
    b, H, W, c = SHAPES[name][:4]
    if job == "crop":                                     # window in + working size out, image and the one-frame mask
        return 4 * (b * c + 1) * (r.h * r.w + r.oh * r.ow)
    halo = (r.h + 2 * (K - 1)) * (r.w + 2 * (K - 1))      # stitch: frame in + frame out + window terms
    return 4 * (2 * b * H * W * c + b * c * (r.oh * r.ow + 4 * r.h * r.w) + b * halo)


def run_shape(name, iters, warmup, filter, new_only=False, only=None):
    import torch
    dev = torch.device("cuda", 0)
    args = make_job(name, filter, dev) + (filter,)
    series = {}
    for job, (new, old) in JOBS.items():
        if only and job != only:
            continue
        fns = [("new_a", new), ("new_b", new)] if new_only else [("new_a", new), ("old_a", old), ("new_b", new), ("old_b", old)]
        for _ in range(warmup):
            for _, fn in fns:
                fn(*args)
        torch.cuda.synchronize()
        rec = {label: [] for label, _ in fns}
        for _ in range(iters):
            for label, fn in fns:
                rec[label].append(timed(fn, args))
        series[job] = rec
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
    out = {k: {"calls": len(v), "total_us": round(sum(v), 2), "median_us": round(statistics.median(v), 2)} for k, v in per.items()}
    anchor = "stitch" if job == "stitch" else "resample"
    if anchor not in per:
        return out, None
    calls = len(per[anchor]) / (1 if job == "stitch" else 2)
    return out, sum(sum(v) for k, v in per.items() if k != "bbox") / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--filter", choices=("bilinear", "bicubic"), default="bicubic")
    ap.add_argument("--shape", choices=sorted(SHAPES))
    ap.add_argument("--job", choices=sorted(JOBS), help="with --shape: run this job only")
    ap.add_argument("--kernels", nargs="*", default=[], help="SHAPE:JOB=rocprofv3 results .db or kernel-trace .csv")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_detailer.py needs a HIP device")
    if a.shape:
        run_shape(a.shape, a.iters, a.warmup, a.filter, new_only=True, only=a.job)
        return
    profiles = dict(kv.split("=", 1) for kv in a.kernels)
    result = {"metric": "detailer_crop_stitch", "unit": "ms", "iters": a.iters, "warmup": a.warmup, "filter": a.filter,
              "blend_overlap": K, "device": torch.cuda.get_device_name(0), "shapes": {}}
    med = statistics.median
    for name in sorted(SHAPES):
        region, series = run_shape(name, a.iters, a.warmup, a.filter)
        rec = {"image": list(SHAPES[name][:4]), "region": [region.y0, region.x0, region.h, region.w],
               "working_size": [region.oh, region.ow]}
        for job, s in series.items():
            new, old = med(s["new_a"] + s["new_b"]), med(s["old_a"] + s["old_b"])
            rec[job] = {"new_ms": round(new, 4), "old_ms": round(old, 4), "old_over_new": round(old / new, 3),
                        "new_min_max_ms": [round(min(s["new_a"] + s["new_b"]), 4), round(max(s["new_a"] + s["new_b"]), 4)],
                        "old_min_max_ms": [round(min(s["old_a"] + s["old_b"]), 4), round(max(s["old_a"] + s["old_b"]), 4)],
                        "spread_new": round(abs(med(s["new_a"]) - med(s["new_b"])) / new, 4),
                        "spread_old": round(abs(med(s["old_a"]) - med(s["old_b"])) / old, 4),
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
        result["shapes"][name] = rec
        torch.cuda.empty_cache()
    print(json.dumps(result, separators=(",", ":")))


if __name__ == "__main__":
    main()
