#!/usr/bin/env python3
"""Tracked Detailer benchmark (lanpaint_amd.detail on the HIP device): one JSON line.

The clip: 81 x 720 x 1280 x 3, an 81-frame mask, one disc of radius 60 (a ~120-pixel subject) that moves 800 pixels across the
frame at constant speed; context 1.5, padding 32, target 512, smooth 9, blend_overlap 9.  Image, mask and detailed crops are
already on the device.

(a) Working pixels: what the sampler is handed per frame (oh x ow) and how many source pixels stand behind them (h x w), for
    plan_track against plan_region on the union box with the same context / padding / target.  Host arithmetic on the boxes.
(b) Times, tracked against a FIXED window of the same (h, w, oh, ow) through the existing single-window calls -- the same bytes
    moved, no per-block table lookup: the yardstick.
        bbox    detail.mask_bbox_frames(mask)                 vs  detail.mask_bbox(mask): the same bytes of mask read once
        crop    detail.crop_track(image, mask, track)         vs  detail.crop_resample(image, mask, fixed region)
        stitch  detail.stitch_track(original, crops, ...)     vs  detail.stitch(original, crops, mask, fixed region)

    python scripts/bench_detailer_track.py [--iters 30] [--warmup 5] [--filter bicubic]
    python scripts/bench_detailer_track.py --job stitch --iters 10      # the body of a rocprofv3 --kernel-trace run

Time: featurebench.events per call; every iteration runs track, fixed, track, fixed, and `fixed_spread` is the margin a
track-vs-fixed difference has to exceed to mean anything.  `bbox` includes the table's device -> host read on both sides.
"""
from __future__ import annotations

import featurebench as fb

FRAMES, H, W, C = 81, 720, 1280, 3
RADIUS, X_FROM, X_TO = 60, 240, 1040
CONTEXT, PADDING, TARGET, SMOOTH, K = 1.5, 32, 512, 9, 9


def clip_mask():
    import torch
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    mask = torch.zeros(FRAMES, H, W)
    for f in range(FRAMES):
        cx = X_FROM + (X_TO - X_FROM) * f // (FRAMES - 1)
        mask[f] = ((yy - H // 2) ** 2 + (xx - cx) ** 2 < RADIUS * RADIUS).float()
    return mask


def make_job(filter, dev):
    import torch
    from lanpaint_amd import detail
    g = torch.Generator(device="cpu").manual_seed(0)
    image = torch.rand(FRAMES, H, W, C, generator=g).to(dev)
    mask = clip_mask().to(dev)
    boxes = detail.mask_bbox_frames(mask)
    track = detail.plan_track(boxes, H, W, CONTEXT, PADDING, 8, TARGET, SMOOTH)
    union = detail.plan_region(detail.mask_bbox(mask), H, W, CONTEXT, PADDING, 8, TARGET)
    fixed = track.region(FRAMES // 2)                              # the same h, w, oh, ow at one place for every frame
    det = torch.rand(FRAMES, track.oh, track.ow, C, generator=g).to(dev)
    return {"image": image, "mask": mask, "boxes": boxes, "track": track, "union": union, "fixed": fixed, "det": det,
            "filter": filter}


def working_pixels(job):
    t, u = job["track"], job["union"]
    side = max(b[3] - b[2] + 1 for b in job["boxes"])
    return {"subject_side": side,
            "track": {"window": [t.h, t.w], "working_size": [t.oh, t.ow], "working_pixels_per_frame": t.oh * t.ow,
                      "source_pixels_per_frame": t.h * t.w, "scale": round(t.ow / t.w, 4),
                      "subject_working_side": round(side * t.ow / t.w, 1), "distinct_origins": len(set(t.origins)),
                      "first_last_origin": [list(t.origins[0]), list(t.origins[-1])]},
            "union": {"window": [u.h, u.w], "working_size": [u.oh, u.ow], "working_pixels_per_frame": u.oh * u.ow,
                      "source_pixels_per_frame": u.h * u.w, "scale": round(u.ow / u.w, 4),
                      "subject_working_side": round(side * u.ow / u.w, 1)},
            "source_pixels_union_over_track": round(u.h * u.w / (t.h * t.w), 3)}


def bbox_track(j):
    from lanpaint_amd import detail
    return detail.mask_bbox_frames(j["mask"])


def bbox_fixed(j):
    from lanpaint_amd import detail
    return detail.mask_bbox(j["mask"])


def crop_track(j):
    from lanpaint_amd import detail
    return detail.crop_track(j["image"], j["mask"], j["track"], j["filter"])


def crop_fixed(j):
    from lanpaint_amd import detail
    return detail.crop_resample(j["image"], j["mask"], j["fixed"], j["filter"])


def stitch_track(j):
    from lanpaint_amd import detail
    return detail.stitch_track(j["image"], j["det"], j["mask"], j["track"], K, j["filter"])


def stitch_fixed(j):
    from lanpaint_amd import detail
    return detail.stitch(j["image"], j["det"], j["mask"], j["fixed"], K, j["filter"])


JOBS = {"bbox": (bbox_track, bbox_fixed), "crop": (crop_track, crop_fixed), "stitch": (stitch_track, stitch_fixed)}


def run(job, iters, warmup, only=None):
    series = {}
    for label, pair in JOBS.items():
        if only and label != only:
            continue
        track, fixed = (lambda f=f: f(job) for f in pair)
        series[label] = fb.series([("track_a", track), ("fixed_a", fixed), ("track_b", track), ("fixed_b", fixed)], iters, warmup)
    return series


def main():
    ap = fb.parser(jobs=sorted(JOBS), iters=30, warmup=5)
    ap.add_argument("--filter", choices=("bilinear", "bicubic"), default="bicubic")
    a = ap.parse_args()
    job = make_job(a.filter, fb.device())
    if a.job:
        run(job, a.iters, a.warmup, only=a.job)
        return
    result = {"filter": a.filter, "blend_overlap": K, "smooth": SMOOTH, "image": [FRAMES, H, W, C], "working_pixels": working_pixels(job)}
    med = fb.median
    for label, s in run(job, a.iters, a.warmup).items():
        track, fixed = med(s["track_a"] + s["track_b"]), med(s["fixed_a"] + s["fixed_b"])
        result[label] = {"track_ms": round(track, 4), "fixed_ms": round(fixed, 4), "track_over_fixed": round(track / fixed, 4),
                         "track_min_max_ms": fb.summary(s["track_a"] + s["track_b"])[1],
                         "fixed_min_max_ms": fb.summary(s["fixed_a"] + s["fixed_b"])[1],
                         "track_spread": fb.spread(s["track_a"], s["track_b"]),
                         "fixed_spread": fb.spread(s["fixed_a"], s["fixed_b"])}
    fb.emit("detailer_track", a, **result)


if __name__ == "__main__":
    main()
