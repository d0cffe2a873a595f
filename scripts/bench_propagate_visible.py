#!/usr/bin/env python3
"""Occlusion-aware video mask propagate benchmark (lanpaint_amd.propagate_visible on the HIP device): one JSON line.

The two workloads of scripts/bench_propagate.py at the default parameters (levels 4, search 2, smooth 8, occlusion 16), key frame
0, everything already on the device, with a static textured bar a twentieth of the width wide drawn over every frame in the disc's
path, so that the occlusion test has something to find:

    clip    81 frames of 1280 x 720 x 3
    square  16 frames of 1024 x 1024 x 3

    whole     propagate_visible.propagate_masks_visible against propagate.propagate_masks on the same clip in the same process,
              alternating, each with featurebench.wall.  Their ratio is the figure that matters.
    stages    lp_prop_visible and lp_prop_occlude alone on the buffers of the clip's first step, featurebench.events over `reps`
              back-to-back calls, next to the step's other launches (match and fill per level, advance) timed the same way.
    torch     the same rule in torch operators on the same device, compared element by element with the module's two outputs, on
              `--torch-frames` frames of the case.

    python scripts/bench_propagate_visible.py [--iters 5] [--warmup 1] [--case clip] [--torch-frames 4]
"""
from __future__ import annotations

import featurebench as fb

import bench_propagate as base  # the clip, the plain rule in torch

LEVELS, SEARCH, SMOOTH, OCCLUSION = base.LEVELS, base.SEARCH, base.SMOOTH, 16


def make_job(case, dev, frames=None):
    import torch
    job = base.make_job(case, dev, frames)
    F, H, W = job["shape"]
    g = torch.Generator(device="cpu").manual_seed(1)
    x0, x1 = W // 2, W // 2 + W // 20
    job["images"][:, :, x0:x1] = torch.rand(H, x1 - x0, 3, generator=g).to(dev)
    job["bar"] = (x0, x1)
    return job


# ---- the same rule in torch operators ----------------------------------------------------------------------------------------------------
def torch_visible_flags(Yt, Yk, P, m, occlusion):
    import torch
    H, W = Yt.shape
    dev = Yt.device
    gh, gw = (H + 7) // 8, (W + 7) // 8
    d = Yt - ((base._bil(Yk, P[..., 0], P[..., 1]) + 128) >> 8)
    r = torch.arange(16, device=dev)
    ys = (torch.arange(gh, device=dev)[:, None] * 8 - 4 + r[None, :])[:, None, :, None]
    xs = (torch.arange(gw, device=dev)[:, None] * 8 - 4 + r[None, :])[None, :, None, :]
    inside = (ys >= 0) & (ys < H) & (xs >= 0) & (xs < W)
    flat = ys.clamp(0, H - 1) * W + xs.clamp(0, W - 1)
    mm = m.reshape(-1)[flat] * inside
    dd = d.reshape(-1)[flat]
    n = mm.sum(dim=(2, 3))
    D = (dd * mm).sum(dim=(2, 3))
    mu = base._floor_div(2 * D + n, (2 * n).clamp(min=1)).clamp(-32, 32)
    R = ((dd - mu[:, :, None, None]).abs() * mm).sum(dim=(2, 3))
    return ((n >= 16) & (R > occlusion * n)).long()


def torch_weight(flags, H, W):
    import torch
    gh, gw = flags.shape
    dev = flags.device

    def axis(n, g):
        u = 2 * torch.arange(n, device=dev) - 7
        b0 = u >> 4
        return b0.clamp(0, g - 1), (b0 + 1).clamp(0, g - 1), u - 16 * b0
    y0, y1, fy = axis(H, gh)
    x0, x1, fx = axis(W, gw)
    fy, fx = fy[:, None], fx[None, :]
    v = 1 - flags
    return (16 - fy) * ((16 - fx) * v[y0][:, x0] + fx * v[y0][:, x1]) + fy * ((16 - fx) * v[y1][:, x0] + fx * v[y1][:, x1])


def torch_propagate_visible(images, mask, levels=LEVELS, search=SEARCH, smooth=SMOOTH, occlusion=OCCLUSION):
    """propagate_masks_visible with key frame 0 in torch operators: (mask, hidden) fp32 [F, H, W]."""
    import torch
    F, H, W = images.shape[:3]
    key = (mask >= 0.5).long()
    Y = base.torch_luma(images)
    yy, xx = torch.meshgrid(torch.arange(H, device=images.device), torch.arange(W, device=images.device), indexing="ij")
    P, bits = torch.stack([16 * yy, 16 * xx], dim=-1), key
    out, hidden = [key.float()], [torch.zeros_like(key, dtype=torch.float32)]
    src = base._pyr(Y[0], levels, True)
    for t in range(1, F):
        tgt, mp, parent = base._pyr(Y[t], levels, True), base._pyr(bits, levels, False), None
        for lv in range(levels - 1, -1, -1):
            parent = base.torch_fill_median(*base.torch_match(src[lv], tgt[lv], mp[lv], parent, search, smooth, lv == 0))
        P, c = base.torch_advance(P, parent, key)
        flags = torch_visible_flags(Y[t], Y[0], P, (c >= 128).long(), occlusion)
        cv = (c * torch_weight(flags, H, W) + 128) >> 8
        out.append(cv.float() / 256.0)
        hidden.append((c - cv).float() / 256.0)
        bits, src = (cv >= 128).long(), tgt
    return torch.stack(out), torch.stack(hidden)


# ---- timing ------------------------------------------------------------------------------------------------------------------------------
def stage_times(job, reps):
    """The step's launches alone on the first step's buffers: ms per call."""
    import torch
    from lanpaint_amd import propagate, propagate_visible as pv
    F, H, W = job["shape"]
    out = {}
    pyr = propagate.luma_pyramids(job["images"][:2], LEVELS)
    mpyr, _ = propagate.key_mask(job["mask"], LEVELS)
    step = propagate.Step(H, W, LEVELS, SEARCH, SMOOTH, job["images"].device, split=(pv.visible_flags, pv.occlude, OCCLUSION))
    step.field_of(pyr[0], pyr[1], mpyr)
    for lv in range(LEVELS - 1, -1, -1):
        parent = None if lv == LEVELS - 1 else step.field[lv + 1]
        out[f"match_level{lv}"] = fb.events(lambda: propagate.match_level(pyr[0], pyr[1], mpyr, H, W, LEVELS, lv, SEARCH, SMOOTH, parent,
                                                                            step.raw[lv], step.valid[lv]), reps)
        out[f"fill_level{lv}"] = fb.events(lambda: propagate.fill_median(step.raw[lv], step.valid[lv], step.field[lv]), reps)
    key_bits = propagate.level_view(mpyr, H, W, 0)[0]
    adv = lambda: propagate.advance(step.field[0], None, key_bits, LEVELS, step.pos[0], step.code, step.raw_mpyr)    # noqa: E731
    out["advance"] = fb.events(adv, reps)
    luma_t, luma_k = (propagate.level_view(pyr[i:i + 1], H, W, 0)[0] for i in (1, 0))
    bits = propagate.level_view(step.raw_mpyr, H, W, 0)[0]
    out["visible"] = fb.events(lambda: pv.visible_flags(step.pos[0], luma_t, luma_k, bits, OCCLUSION, step.flags), reps)
    o, h = (torch.empty((H, W), dtype=torch.float32, device=bits.device) for _ in range(2))
    out["occlude"] = fb.events(lambda: pv.occlude(step.code, step.flags, LEVELS, o, h, step.mpyr[0]), reps)
    torch.cuda.synchronize()
    return out, int(step.flags.sum()), step.flags.numel()


def measure(job, iters, warmup, torch_frames, reps):
    from lanpaint_amd import propagate, propagate_visible as pv
    F, H, W = job["shape"]
    new = lambda: pv.propagate_masks_visible(job["images"], job["mask"], 0, LEVELS, SEARCH, SMOOTH, OCCLUSION)    # noqa: E731
    old = lambda: propagate.propagate_masks(job["images"], job["mask"], 0, LEVELS, SEARCH, SMOOTH)               # noqa: E731
    got, hid = new()
    plain = old()
    x0, x1 = job["bar"]
    on_bar, on_bar_plain = int((got[:, :, x0:x1] >= 0.5).sum()), int((plain[:, :, x0:x1] >= 0.5).sum())
    differing_again = fb.differing(new(), (got, hid))
    n = min(torch_frames, F)
    eager = lambda: torch_propagate_visible(job["images"][:n], job["mask"])                                                      # noqa: E731
    small = lambda: pv.propagate_masks_visible(job["images"][:n], job["mask"], 0, LEVELS, SEARCH, SMOOTH, OCCLUSION)             # noqa: E731
    differing = fb.differing(eager(), small())
    del plain
    # alternating: the two share whatever else the host does
    fb.untimed(lambda: (new(), old()), warmup)
    s = fb.series([("new", new), ("old", old), ("torch", eager), ("small", small)], iters, 0, timer=fb.wall)
    new_ms, old_ms, torch_ms, small_ms = s.values()
    stages, flagged, blocks = stage_times(job, reps)
    med = fb.median
    match_fill = sum(v for k, v in stages.items() if k.startswith(("match", "fill")))
    return {"case": job["case"], "frames_height_width": [F, H, W], "levels": LEVELS, "search": SEARCH, "smooth": SMOOTH,
            "occlusion": OCCLUSION, "visible_wall_ms": round(med(new_ms), 3),
            "visible_wall_min_max_ms": fb.summary(new_ms, 3)[1],
            "plain_wall_ms": round(med(old_ms), 3), "plain_wall_min_max_ms": fb.summary(old_ms, 3)[1],
            "visible_over_plain": round(med(new_ms) / med(old_ms), 3),
            "stage_ms": {k: round(v, 5) for k, v in stages.items()}, "stage_reps": reps,
            "new_launches_ms_per_step": round(stages["visible"] + stages["occlude"], 5),
            "match_and_fill_ms_per_step": round(match_fill, 5), "advance_ms_per_step": round(stages["advance"], 5),
            "first_step_blocks_flagged": [flagged, blocks],
            "mask_pixels_on_bar": on_bar, "mask_pixels_on_bar_plain": on_bar_plain, "hidden_mass": round(float(hid.sum()), 1),
            "elements_differing_between_two_calls": differing_again,
            "torch_frames": n, "torch_ms": round(med(torch_ms), 3), "module_ms_same_frames": round(med(small_ms), 3),
            "torch_over_module": round(med(torch_ms) / med(small_ms), 2), "elements_differing_from_torch": differing}


def main():
    ap = fb.parser(base.CASES, iters=5, warmup=1)
    ap.add_argument("--reps", type=int, default=50, help="back-to-back calls per stage timing")
    ap.add_argument("--torch-frames", type=int, default=4)
    a = ap.parse_args()
    dev = fb.device()
    import torch
    results = []
    for case in ((a.case,) if a.case else tuple(base.CASES)):
        job = make_job(case, dev)
        results.append(measure(job, a.iters, a.warmup, a.torch_frames, a.reps))
        del job
        torch.cuda.empty_cache()
    fb.emit("mask_propagate_visible", a, results)


if __name__ == "__main__":
    main()
