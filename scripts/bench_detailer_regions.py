#!/usr/bin/env python3
"""Per-region Detailer benchmark (lanpaint_amd.detail on the HIP device): one JSON line.

Shapes (image, mask and detailed crops already on the device; mask discs as (cy, cx, r)):
    clip   81 x 720 x 1280 x 3, an 81-frame mask, two discs  -> 2 regions, worked at 512 long side
    still  1 x 2160 x 3840 x 3, a 1-frame mask, three discs  -> 3 regions, worked at 1024 long side

Jobs, new against what the tree had before for the same result:
    label   detail.mask_components(mask)                  vs  detail.mask_bbox(mask): the same bytes of mask read once
    crop    detail.crop_regions(image, mask, regions)     vs  detail.crop_resample once per region, with that region's mask
    stitch  detail.stitch_regions(original, crops, ...)   vs  detail.stitch composed over the regions

    python scripts/bench_detailer_regions.py [--iters 30] [--warmup 5] [--filter bicubic] [--kernels clip=A.db still=B.db]
    python scripts/bench_detailer_regions.py --shape clip --job label --iters 10   # the body of a rocprofv3 --kernel-trace run

Time: featurebench.events per call; every iteration runs new, old, new, old.  `label` includes the table's device -> host
read on both sides (mask_bbox reads its four integers back too).  Per-kernel times come from a SEPARATE rocprofv3 --kernel-trace
--stats run of `--shape S --job label`, which runs mask_components and mask_bbox alternately (--kernels reads its results .db /
kernel-trace CSV): per launch the median and min-max, the bytes the launch has to touch, and the union pass against
lp_detail_bbox_kernel on the same input in that run.
"""
from __future__ import annotations

import featurebench as fb

COPY_ACHIEVABLE = 6.29e12
# name: (B, mask frames, H, W, C, discs (cy, cx, r), context, padding, target)
SHAPES = {"clip": (81, 81, 720, 1280, 3, ((200, 300, 60), (500, 1000, 80)), 1.5, 32, 512),
          "still": (1, 1, 2160, 3840, 3, ((500, 700, 150), (1500, 3000, 200), (1800, 600, 120)), 1.5, 32, 1024)}
K = 9
LABEL_KERNELS = ("union", "tile", "border", "flatten", "scan", "rank", "relabel")


def make_job(name, filter, dev):
    import torch
    from lanpaint_amd import detail
    b, mb, H, W, c, discs, context, padding, target = SHAPES[name]
    g = torch.Generator(device="cpu").manual_seed(0)
    image = torch.rand(b, H, W, c, generator=g).to(dev)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    mask = torch.zeros(mb, H, W)
    for i, (cy, cx, r) in enumerate(discs):                        # every disc in every frame, drifting a pixel per frame
        for f in range(mb):
            mask[f] = torch.maximum(mask[f], ((yy - cy) ** 2 + (xx - cx - f % 8) ** 2 < r * r).float())
    mask = mask.to(dev)
    labels, n, table = detail.mask_components(mask)
    regions = detail.plan_regions((n, table), H, W, context, padding, 8, target)
    assert len(regions) == len(discs), (len(regions), n)
    det = torch.rand(len(regions) * b, regions.oh, regions.ow, c, generator=g).to(dev)
    region_masks = []
    for mem in regions.members:                                    # what the old path needs: a frame-sized mask per region
        foreign = (labels != 0) & ~torch.isin(labels, torch.tensor(mem, dtype=labels.dtype, device=dev))
        region_masks.append(torch.where(foreign.unsqueeze(0), torch.zeros((), device=dev), mask))
    return {"image": image, "mask": mask, "labels": labels, "regions": regions, "det": det, "region_masks": region_masks,
            "filter": filter}


def label_new(j):
    from lanpaint_amd import detail
    return detail.mask_components(j["mask"])


def label_old(j):
    from lanpaint_amd import detail
    return detail.mask_bbox(j["mask"])


def crop_new(j):
    from lanpaint_amd import detail
    return detail.crop_regions(j["image"], j["mask"], j["regions"], j["labels"], j["filter"])


def crop_old(j):
    from lanpaint_amd import detail
    return [detail.crop_resample(j["image"], m, j["regions"].region(i), j["filter"]) for i, m in enumerate(j["region_masks"])]


def stitch_new(j):
    from lanpaint_amd import detail
    return detail.stitch_regions(j["image"], j["det"], j["mask"], j["regions"], j["labels"], K, j["filter"])


def stitch_old(j):
    from lanpaint_amd import detail
    out, b = j["image"], j["image"].shape[0]
    for i, m in enumerate(j["region_masks"]):
        out = detail.stitch(out, j["det"][i * b:(i + 1) * b], m, j["regions"].region(i), K, j["filter"])
    return out


JOBS = {"label": (label_new, label_old), "crop": (crop_new, crop_old), "stitch": (stitch_new, stitch_old)}


def run_shape(name, iters, warmup, filter, only=None):
    job = make_job(name, filter, fb.device())
    series = {}
    for label, (new, old) in JOBS.items():
        if only and label != only:
            continue
        new, old = (lambda f=f: f(job) for f in (new, old))
        series[label] = fb.series([("new_a", new), ("old_a", old), ("new_b", new), ("old_b", old)], iters, warmup)
    return job, series


def label_launch_bytes(name):
    """Bytes each launch of lp_mask_components has to touch (n = H * W int32 elements, planes of fp32)."""
    _, mb, H, W = SHAPES[name][:4]
    n, chunks = H * W, (H * W + 1023) // 1024
    return {"union": 4 * n * (mb + 1), "tile": 8 * n, "border": 4 * n * (1 / 16 + 2 / 64), "flatten": 4 * n + 4 * chunks,
            "scan": 8 * chunks + 20 * 4096, "rank": 4 * n + 4 * chunks, "relabel": 8 * n, "bbox": 4 * n * mb}


def kernel_stats(path, name):
    from rocprof_summary import rows_from_csv, rows_from_db
    rows = rows_from_db(path) if path.endswith(".db") else rows_from_csv(path)
    per = {}
    for kname, start, end, *_ in rows:
        for k in LABEL_KERNELS:
            if f"lp_label_{k}_kernel" in kname:
                per.setdefault(k, []).append((end - start) * 1e-3)
        if "lp_detail_bbox_kernel" in kname:
            per.setdefault("bbox", []).append((end - start) * 1e-3)
    need = label_launch_bytes(name)
    out = {}
    for k, v in per.items():
        med = fb.median(v)
        out[k] = {"calls": len(v), "median_us": round(med, 2), "min_max_us": [round(min(v), 2), round(max(v), 2)],
                  "bytes": int(need[k]), "copy_rate_frac": round(need[k] / (med * 1e-6) / COPY_ACHIEVABLE, 4)}
    if "union" in out and "bbox" in out:
        out["union_over_bbox"] = round(out["union"]["median_us"] / out["bbox"]["median_us"], 3)
        out["bbox_spread"] = round((out["bbox"]["min_max_us"][1] - out["bbox"]["min_max_us"][0]) / out["bbox"]["median_us"], 3)
    out["launches_total_us"] = round(sum(out[k]["median_us"] for k in LABEL_KERNELS if k in out), 2)
    return out


def main():
    ap = fb.parser(iters=30, warmup=5)
    ap.add_argument("--filter", choices=("bilinear", "bicubic"), default="bicubic")
    ap.add_argument("--shape", choices=sorted(SHAPES))
    ap.add_argument("--job", choices=sorted(JOBS), help="with --shape: run this job only")
    ap.add_argument("--kernels", nargs="*", default=[], help="SHAPE=rocprofv3 results .db or kernel-trace .csv of a label run")
    a = ap.parse_args()
    fb.device()
    import torch
    if a.shape:
        run_shape(a.shape, a.iters, a.warmup, a.filter, only=a.job)
        return
    profiles = dict(kv.split("=", 1) for kv in a.kernels)
    shapes = {}
    med = fb.median
    for name in sorted(SHAPES):
        job, series = run_shape(name, a.iters, a.warmup, a.filter)
        g = job["regions"]
        rec = {"image": list(job["image"].shape), "mask_frames": job["mask"].shape[0], "regions": len(g),
               "window": [g.h, g.w], "working_size": [g.oh, g.ow], "origins": [list(o) for o in g.origins]}
        for label, s in series.items():
            new, old = med(s["new_a"] + s["new_b"]), med(s["old_a"] + s["old_b"])
            rec[label] = {"new_ms": round(new, 4), "old_ms": round(old, 4), "old_over_new": round(old / new, 3),
                          "new_min_max_ms": fb.summary(s["new_a"] + s["new_b"])[1],
                          "old_min_max_ms": fb.summary(s["old_a"] + s["old_b"])[1],
                          "spread_new": fb.spread(s["new_a"], s["new_b"]),
                          "spread_old": fb.spread(s["old_a"], s["old_b"])}
        rec["label"]["kernels"] = kernel_stats(profiles[name], name) if name in profiles else "not measured"
        shapes[name] = rec
        del job
        torch.cuda.empty_cache()
    fb.emit("detailer_regions", a, filter=a.filter, blend_overlap=K, shapes=shapes)


if __name__ == "__main__":
    main()
