#!/usr/bin/env python3
"""Video mask editor benchmark (lanpaint_amd.videomask.interpolate_masks on the HIP device): one JSON line.

Shapes (keyframes already on the device, as a node that keeps them there would hold them):
    a  2 keyframes 480x832 -> 81 frames at 1280x720
    b  4 keyframes 480x832 -> 121 frames at 1920x1080
    c  2 keyframes 480x832 -> 81 frames, identity size (no resize)

    python scripts/bench_videomask.py [--iters 30] [--warmup 5] [--kernels a=A.db b=B.db c=C.db]
    python scripts/bench_videomask.py --shape a --iters 5          # the body of a rocprofv3 --kernel-trace run

Time: featurebench.wall per call, median over --iters after --warmup.  Per-kernel
times come from a SEPARATE rocprofv3 --kernel-trace --stats run per shape (--kernels reads its results .db / kernel-trace
CSV); the resize kernel's output bytes over its mean time are reported against 6.3 TB/s achievable HBM bandwidth.
"""
from __future__ import annotations

import featurebench as fb

HBM_ACHIEVABLE = 6.3e12
SHAPES = {"a": (2, 81, (1280, 720)), "b": (4, 121, (1920, 1080)), "c": (2, 81, None)}
KEY_H, KEY_W = 480, 832


def keyframes(n, count, dev):
    import numpy as np
    import torch
    yy, xx = np.mgrid[:KEY_H, :KEY_W].astype(np.float64)
    out = {}
    for j in range(n):
        t = round(j * (count - 1) / (n - 1))
        cy, cx, r = 180 + 60 * j, 220 + 140 * j, 80 + 25 * (j % 3)
        d = np.sqrt((yy - cy) ** 2 + (xx - cx) ** 2) - r
        m = np.round(np.clip(0.5 - d / 6.0, 0.0, 1.0) * 255.0) / 255.0
        out[t] = torch.from_numpy(m.astype(np.float32)).to(dev)
    return out


def run_shape(name, iters, warmup):
    from lanpaint_amd import videomask
    dev = fb.device()
    n, count, size = SHAPES[name]
    keys = keyframes(n, count, dev)
    call = lambda: videomask.interpolate_masks(keys, count, size=size, device=dev)    # noqa: E731
    return fb.series([("wall", call)], iters, warmup, timer=fb.wall)["wall"]


def kernel_stats(path):
    from rocprof_summary import rows_from_csv, rows_from_db
    rows = rows_from_db(path) if path.endswith(".db") else rows_from_csv(path)
    per = {}
    for name, start, end, *_ in rows:
        for k in ("col", "row", "sdf", "morph", "resize"):
            if f"lp_vmask_{k}_kernel" in name:
                per.setdefault(k, []).append((end - start) * 1e-3)
    return {k: {"calls": len(v), "mean_us": round(sum(v) / len(v), 2), "median_us": round(fb.median(v), 2)}
            for k, v in per.items()}


def main():
    ap = fb.parser(iters=30, warmup=5)
    ap.add_argument("--shape", choices=sorted(SHAPES))
    ap.add_argument("--kernels", nargs="*", default=[], help="SHAPE=rocprofv3 results .db or kernel-trace .csv")
    args = ap.parse_args()
    fb.device()
    import torch
    if args.shape:
        run_shape(args.shape, args.iters, args.warmup)
        return
    profiles = dict(kv.split("=", 1) for kv in args.kernels)
    shapes = {}
    for name in sorted(SHAPES):
        n, count, size = SHAPES[name]
        times = run_shape(name, args.iters, args.warmup)
        w, h = size or (KEY_W, KEY_H)
        ms, (low, high) = fb.summary(times)
        rec = {"keys": n, "frames": count, "out": [count, h, w], "out_bytes": count * h * w * 4,
               "wall_ms_median": ms, "wall_ms_min": low, "wall_ms_max": high}
        if name in profiles:
            ks = kernel_stats(profiles[name])
            rec["kernels"] = ks
            big = ks.get("resize") or ks.get("morph")
            if big:
                rec["big_kernel"] = "resize" if "resize" in ks else "morph"
                rec["big_kernel_hbm_frac"] = round(rec["out_bytes"] / (big["median_us"] * 1e-6) / HBM_ACHIEVABLE, 4)
        else:
            rec["kernels"] = "not measured"
        shapes[name] = rec
        torch.cuda.empty_cache()
    fb.emit("videomask_interpolate_masks", args, shapes=shapes)


if __name__ == "__main__":
    main()
