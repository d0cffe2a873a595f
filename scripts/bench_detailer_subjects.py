#!/usr/bin/env python3
"""Per-subject Detailer benchmark (lanpaint_amd.detail_subjects on the HIP device): one JSON line.

The clip: 81 x 720 x 1280 x 3 with an 81-frame mask of three discs: two of radius 60 (~120-pixel subjects) that cross the frame
in opposite directions on different rows, so their paths cross and their masks never touch, and one of radius 20 that appears
in frame 60.  context 1.5, padding 32, target 512, smooth 9, blend_overlap 9, min_area 64, max_subjects 4.  Image, mask and
detailed crops are already on the device.

(a) Working pixels, host arithmetic only: the window and the working pixels per subject under plan_track (one box per frame,
    which spans every subject in it) against plan_subjects.  `--host-only` prints this part from numpy boxes without a device.
(b) Kernel resources come from the library's metadata (scripts/instantiation_coverage.py kernel_resources), not from here.
(c) Times against yardsticks in the same process, interleaved (featurebench.events per call; every iteration runs new,
    yardstick, new, yardstick, and `yard_spread` is the margin a difference has to exceed):
        label   lp_mask_components_frames on the volume   vs  `frames` back-to-back lp_mask_components calls on single frames
                (raw entries into preallocated buffers on both sides, no table read-back inside the timed span)
        crop    detail_subjects.crop_subjects             vs  detail.crop_track called S times, once per subject's path
        stitch  detail_subjects.stitch_subjects           vs  detail.stitch_track called S times, chained

    Bytes, per voxel of the volume (DESIGN.md section 4's table): the seven launches move 8 (threshold: read the mask, write
    P) + 8 (tile) + 0.5 (border) + 4 (flatten) + 4 (rank) + 8 (relabel) = 32.5 bytes; the temporal launch reads each voxel's
    parent in frames 1 .. F - 1 and the parent below it: 8 (F - 1) / F bytes.  Expected label ratio on bytes:
    (32.5 + 8 * 80 / 81) / 32.5 = 1.24.  The yardstick also pays 7 x 81 launches against 8, each over a frame too small to
    hide its launch, so the measured ratio may sit well below the bytes'.

    python scripts/bench_detailer_subjects.py [--iters 20] [--warmup 3] [--filter bicubic]
    python scripts/bench_detailer_subjects.py --host-only
"""
from __future__ import annotations

import json

import featurebench as fb

FRAMES, H, W, C = 81, 720, 1280, 3
DISCS = ((60, 250, 240, 1040, 0), (60, 470, 1040, 240, 0), (20, 360, 600, 680, 60))   # radius, row, x from, x to, first frame
CONTEXT, PADDING, TARGET, SMOOTH, K, MIN_AREA, MAX_SUBJECTS = 1.5, 32, 512, 9, 9, 64, 4
EXPECTED_LABEL_RATIO = (32.5 + 8.0 * (FRAMES - 1) / FRAMES) / 32.5


def disc_masks():
    """One bool volume [FRAMES, H, W] per disc, numpy."""
    import numpy as np
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for radius, cy, x_from, x_to, first in DISCS:
        vol = np.zeros((FRAMES, H, W), bool)
        for f in range(first, FRAMES):
            cx = x_from + (x_to - x_from) * (f - first) // max(FRAMES - 1 - first, 1)
            vol[f] = (yy - cy) ** 2 + (xx - cx) ** 2 < radius * radius
        out.append(vol)
    return out


def host_boxes(vol):
    import numpy as np
    boxes = []
    for plane in vol:
        ys, xs = np.nonzero(plane.any(1))[0], np.nonzero(plane.any(0))[0]
        boxes.append((int(ys[0]), int(ys[-1]), int(xs[0]), int(xs[-1])) if ys.size else (H, -1, W, -1))
    return tuple(boxes)


def plans(per_subject_boxes, frame_boxes):
    from lanpaint_amd import detail, detail_subjects
    members = tuple((s + 1,) for s in range(len(per_subject_boxes)))
    subjects = detail_subjects.plan_subjects(members, per_subject_boxes, H, W, CONTEXT, PADDING, 8, TARGET, SMOOTH)
    track = detail.plan_track(frame_boxes, H, W, CONTEXT, PADDING, 8, TARGET, SMOOTH)
    return subjects, track


def working_pixels(per_subject_boxes, subjects, track):
    rows = []
    for s, boxes in enumerate(per_subject_boxes):
        side = max(b[3] - b[2] + 1 for b in boxes if b[1] >= b[0])
        rows.append({"subject": s, "side": side,
                     "track": {"window": [track.h, track.w], "working_size": [track.oh, track.ow],
                               "subject_working_side": round(side * track.ow / track.w, 1)},
                     "subjects": {"window": [subjects.h, subjects.w], "working_size": [subjects.oh, subjects.ow],
                                  "subject_working_side": round(side * subjects.ow / subjects.w, 1)}})
    return {"per_subject": rows, "track_batch": track.oh * track.ow * FRAMES,
            "subjects_batch": subjects.oh * subjects.ow * FRAMES * subjects.subjects,
            "source_pixels_track_over_subjects": round(track.h * track.w / (subjects.h * subjects.w), 3)}


def make_job(filter, dev):
    import numpy as np
    import torch
    from lanpaint_amd import _cabi, detail, detail_subjects
    vols = disc_masks()
    mask = torch.from_numpy(np.logical_or.reduce(vols)).float().to(dev)
    g = torch.Generator(device="cpu").manual_seed(0)
    image = torch.rand(FRAMES, H, W, C, generator=g).to(dev)
    labels, n, table = detail_subjects.mask_components_frames(mask)
    members = detail_subjects.group_subjects((n, table), MIN_AREA, MAX_SUBJECTS)
    boxes = detail_subjects.subject_boxes(labels, members)
    assert n == len(DISCS) and boxes == tuple(host_boxes(v) for v in vols), "the device's boxes are not the scene's"
    frame_boxes = detail.mask_bbox_frames(mask)
    subjects, track = plans(boxes, frame_boxes)
    paths = [detail.Track(H, W, subjects.h, subjects.w, subjects.oh, subjects.ow,
                          subjects.origins[s * FRAMES:(s + 1) * FRAMES]) for s in range(subjects.subjects)]
    det = torch.rand(subjects.subjects * FRAMES, subjects.oh, subjects.ow, C, generator=g).to(dev)
    raw = {"labels3": torch.empty((FRAMES, H, W), dtype=torch.int32, device=dev),
           "table3": torch.empty(1 + 7 * _cabi.LP_DETAIL_MAX_COMPONENTS, dtype=torch.int32, device=dev),
           "ws3": torch.empty(_cabi.lp_components_frames_ws_bytes(FRAMES, H, W) // 4, dtype=torch.int32, device=dev),
           "labels2": torch.empty((H, W), dtype=torch.int32, device=dev),
           "table2": torch.empty(1 + 5 * _cabi.LP_DETAIL_MAX_COMPONENTS, dtype=torch.int32, device=dev),
           "ws2": torch.empty(_cabi.lp_components_ws_bytes(H, W) // 4, dtype=torch.int32, device=dev)}
    return {"image": image, "mask": mask, "labels": labels, "boxes": boxes, "subjects": subjects, "track": track, "paths": paths,
            "det": det, "filter": filter, "raw": raw, "dev": dev}


def label_new(j):
    from lanpaint_amd import _cabi
    from lanpaint_amd._util import raw_stream
    r = j["raw"]
    _cabi.check(_cabi.load().lp_mask_components_frames(j["mask"].data_ptr(), FRAMES, H, W, r["labels3"].data_ptr(),
                                                       r["table3"].data_ptr(), r["ws3"].data_ptr(), r["ws3"].numel() * 4,
                                                       raw_stream(j["dev"])), "lp_mask_components_frames")


def label_yard(j):
    from lanpaint_amd import _cabi
    from lanpaint_amd._util import raw_stream
    r, lib, stream, base = j["raw"], _cabi.load(), raw_stream(j["dev"]), j["mask"].data_ptr()
    for f in range(FRAMES):
        _cabi.check(lib.lp_mask_components(base + 4 * f * H * W, 1, H, W, r["labels2"].data_ptr(), r["table2"].data_ptr(),
                                           r["ws2"].data_ptr(), r["ws2"].numel() * 4, stream), "lp_mask_components")


def crop_new(j):
    from lanpaint_amd import detail_subjects
    return detail_subjects.crop_subjects(j["image"], j["mask"], j["subjects"], j["labels"], j["filter"])


def crop_yard(j):
    from lanpaint_amd import detail
    return [detail.crop_track(j["image"], j["mask"], path, j["filter"]) for path in j["paths"]]


def stitch_new(j):
    from lanpaint_amd import detail_subjects
    return detail_subjects.stitch_subjects(j["image"], j["det"], j["mask"], j["subjects"], j["labels"], K, j["filter"])


def stitch_yard(j):
    from lanpaint_amd import detail
    out = j["image"]
    for s, path in enumerate(j["paths"]):
        out = detail.stitch_track(out, j["det"][s * FRAMES:(s + 1) * FRAMES], j["mask"], path, K, j["filter"])
    return out


JOBS = {"label": (label_new, label_yard), "crop": (crop_new, crop_yard), "stitch": (stitch_new, stitch_yard)}


def run(job, iters, warmup, only=None):
    series = {}
    for label, pair in JOBS.items():
        if only and label != only:
            continue
        new, yard = (lambda f=f: f(job) for f in pair)
        series[label] = fb.series([("new_a", new), ("yard_a", yard), ("new_b", new), ("yard_b", yard)], iters, warmup)
    return series


def main():
    ap = fb.parser(jobs=sorted(JOBS), iters=20, warmup=3)
    ap.add_argument("--filter", choices=("bilinear", "bicubic"), default="bicubic")
    ap.add_argument("--host-only", action="store_true", help="part (a) from numpy boxes; needs no device")
    a = ap.parse_args()
    result = {"filter": a.filter, "blend_overlap": K, "smooth": SMOOTH, "image": [FRAMES, H, W, C],
              "expected_label_ratio_from_bytes": round(EXPECTED_LABEL_RATIO, 4)}
    if a.host_only:
        import numpy as np
        vols = disc_masks()
        boxes = tuple(host_boxes(v) for v in vols)
        subjects, track = plans(boxes, host_boxes(np.logical_or.reduce(vols)))
        result["working_pixels"] = working_pixels(boxes, subjects, track)
        print(json.dumps({"metric": "detailer_subjects", "unit": "ms", **result}, separators=(",", ":")))
        return
    job = make_job(a.filter, fb.device(hint=" (or --host-only for part (a))"))
    if a.job:
        run(job, a.iters, a.warmup, only=a.job)
        return
    result["working_pixels"] = working_pixels(job["boxes"], job["subjects"], job["track"])
    med = fb.median
    for label, s in run(job, a.iters, a.warmup).items():
        new, yard = med(s["new_a"] + s["new_b"]), med(s["yard_a"] + s["yard_b"])
        result[label] = {"new_ms": round(new, 4), "yard_ms": round(yard, 4), "new_over_yard": round(new / yard, 4),
                         "new_min_max_ms": fb.summary(s["new_a"] + s["new_b"])[1],
                         "yard_min_max_ms": fb.summary(s["yard_a"] + s["yard_b"])[1],
                         "new_spread": fb.spread(s["new_a"], s["new_b"]),
                         "yard_spread": fb.spread(s["yard_a"], s["yard_b"])}
    fb.emit("detailer_subjects", a, **result)


if __name__ == "__main__":
    main()
