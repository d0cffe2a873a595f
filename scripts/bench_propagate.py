#!/usr/bin/env python3
"""Video mask propagate benchmark (lanpaint_amd.propagate on the HIP device): one JSON line.

Two workloads at the default parameters (levels 4, search 2, smooth 8), key frame 0, everything already on the device:

    clip    81 frames of 1280 x 720 x 3: a textured disc that moves (1.5, 4.0) pixels per frame over a texture that moves (-0.5, 1.0)
    square  16 frames of 1024 x 1024 x 3, the same

    whole     propagate.propagate_masks: the luma pyramids per chunk of frames, the key mask, then F - 1 dependent steps of
              2 levels + 1 launches each.  Timed with featurebench.wall, and with featurebench.events.
    stages    every entry on its own, on the buffers of the clip's first step: lp_prop_luma (all frames), lp_prop_key_mask,
              lp_prop_match and lp_prop_fill per level, lp_prop_advance; `reps` back-to-back calls between two device events.
    launches  counted by wrapping the module's launch(): per call and per step.
    gaps      1 - (the stages' times, each times its count in a call) / whole: the share of a call in which the device waits for
              the next launch of the dependent chain.  An estimate from event timings; a kernel trace measures it directly
              (--job whole is the body of such a run).
    torch     the same rule in torch operators on the same device (unfolded windows, gathers, sorts), compared element by element
              with the module's result; on `--torch-frames` frames of the case, since its window tensors are large.

    python scripts/bench_propagate.py [--iters 5] [--warmup 1] [--case clip] [--torch-frames 4]
    python scripts/bench_propagate.py --job whole --case clip --iters 3          # the body of a rocprofv3 --kernel-trace run
"""
from __future__ import annotations

import featurebench as fb

CASES = {"clip": (81, 720, 1280), "square": (16, 1024, 1024)}
LEVELS, SEARCH, SMOOTH = 4, 2, 8


def make_job(case, dev, frames=None):
    import torch
    import torch.nn.functional as Fn
    F, H, W = CASES[case]
    F = frames or F
    g = torch.Generator(device="cpu").manual_seed(0)

    def texture():                                                    # octaves of smooth noise, [3, 2H, 2W] in 0..1
        t = torch.zeros(1, 3, 2 * H, 2 * W)
        for k, amp in ((64, 1.0), (16, 0.5), (4, 0.25), (1, 0.12)):
            n = torch.rand(1, 3, 2 * H // k + 2, 2 * W // k + 2, generator=g)
            t += amp * Fn.interpolate(n, size=(2 * H, 2 * W), mode="bilinear", align_corners=False)
        return ((t - t.min()) / (t.max() - t.min()))[0].to(dev)
    bg, ob = texture(), texture()
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    r, cy0, cx0 = min(H, W) / 5, H / 3, W / 4
    images = torch.empty(F, H, W, 3, device=dev)
    for t in range(F):
        # whole-pixel crops of the two textures at rounded positions: sub-pixel motion comes from the rounding's jitter
        oy, ox = H // 2 - round(-0.5 * t), W // 2 - round(1.0 * t)
        by, bx = H // 2 - round(1.5 * t), W // 2 - round(4.0 * t)
        disc = (yy - cy0 - 1.5 * t) ** 2 + (xx - cx0 - 4.0 * t) ** 2 <= r * r
        frame = torch.where(disc, ob[:, by:by + H, bx:bx + W], bg[:, oy:oy + H, ox:ox + W])
        images[t] = frame.permute(1, 2, 0)
    mask = ((yy - cy0) ** 2 + (xx - cx0) ** 2 <= r * r).float()
    truth = ((yy - cy0 - 1.5 * (F - 1)) ** 2 + (xx - cx0 - 4.0 * (F - 1)) ** 2 <= r * r)
    return {"case": case, "images": images, "mask": mask, "truth": truth, "shape": (F, H, W)}


# ---- the same rule in torch operators ----------------------------------------------------------------------------------------------------
def _down(a, avg):
    import torch.nn.functional as Fn
    h, w = a.shape
    p = Fn.pad(a[None, None].float(), (0, w % 2, 0, h % 2), mode="replicate")[0, 0].long()
    q = p[0::2, 0::2], p[0::2, 1::2], p[1::2, 0::2], p[1::2, 1::2]
    return (q[0] + q[1] + q[2] + q[3] + 2) >> 2 if avg else q[0] | q[1] | q[2] | q[3]


def _pyr(a, levels, avg):
    out = [a.long()]
    for _ in range(levels - 1):
        out.append(_down(out[-1], avg))
    return out


def torch_luma(images):
    import torch
    t = torch.where(images > 0, images.clamp(max=1.0), torch.zeros_like(images))
    q = (t * 255.0 + 0.5).long()
    return (77 * q[..., 0] + 150 * q[..., 1] + 29 * q[..., 2] + 128) >> 8 if q.shape[-1] >= 3 else q[..., 0]


def _floor_div(a, b):
    import torch
    return torch.div(a, b, rounding_mode="floor")


def torch_match(Ys, Yt, m, parent, R, smooth, subpel):
    import torch
    h, w = Ys.shape
    dev = Ys.device
    gh, gw = (h + 7) // 8, (w + 7) // 8
    n = 2 * R + 1
    by, bx = torch.arange(gh, device=dev), torch.arange(gw, device=dev)
    if parent is None:
        p = torch.zeros(gh, gw, 2, dtype=torch.long, device=dev)
    else:
        p = 2 * ((parent[(by >> 1).clamp(max=parent.shape[0] - 1)][:, (bx >> 1).clamp(max=parent.shape[1] - 1)] + 8) >> 4)
    r = torch.arange(16, device=dev)
    ys = (by[:, None] * 8 - 4 + r[None, :])[:, None, :, None]          # [gh, 1, 16, 1]
    xs = (bx[:, None] * 8 - 4 + r[None, :])[None, :, None, :]          # [1, gw, 1, 16]
    inside = (ys >= 0) & (ys < h) & (xs >= 0) & (xs < w)
    flat = ys.clamp(0, h - 1) * w + xs.clamp(0, w - 1)
    mm = m.reshape(-1)[flat] * inside
    win = Ys.reshape(-1)[flat]
    valid = mm.sum(dim=(2, 3)) >= 16
    S = torch.empty(n * n, gh, gw, dtype=torch.long, device=dev)
    keys = torch.empty_like(S)
    py, px = p[..., 0][:, :, None, None], p[..., 1][:, :, None, None]
    for oy in range(-R, R + 1):
        ty = (ys + py + oy).clamp(0, h - 1)
        for ox in range(-R, R + 1):
            tx = (xs + px + ox).clamp(0, w - 1)
            idx, dist = (oy + R) * n + ox + R, abs(oy) + abs(ox)
            S[idx] = ((win - Yt.reshape(-1)[ty * w + tx]).abs() * mm).sum(dim=(2, 3))
            keys[idx] = ((S[idx] + smooth * dist) << 12) | (dist << 8) | idx
    best = keys.min(dim=0).values & 255
    oy, ox = _floor_div(best, n) - R, best % n - R
    v = torch.stack([16 * (p[..., 0] + oy), 16 * (p[..., 1] + ox)], dim=-1)
    if subpel:
        s0 = S.gather(0, best[None])[0]
        for axis, o, step in ((0, oy, n), (1, ox, 1)):
            inner = (o.abs() < R) & (s0 != 0)
            cm = S.gather(0, (best - step).clamp(0, n * n - 1)[None])[0]
            cp = S.gather(0, (best + step).clamp(0, n * n - 1)[None])[0]
            d, g = cm + cp - 2 * s0, cm - cp
            add = torch.sign(g) * torch.minimum(_floor_div((8 * g).abs(), d.clamp(min=1)), torch.full_like(d, 8))
            v[..., axis] += torch.where(inner & (d > 0), add, torch.zeros_like(add))
    v = torch.where(valid[..., None], v, 16 * p)
    return v, valid


def _neigh(a, mode):
    """The nine 3 x 3 neighbours of every cell of a [gh, gw, K]: [9, gh, gw, K]; `mode` replicate, or zeros outside."""
    import torch
    import torch.nn.functional as Fn
    gh, gw = a.shape[:2]
    p = a.permute(2, 0, 1)[None].double()
    p = Fn.pad(p, (1, 1, 1, 1), mode="replicate") if mode == "replicate" else Fn.pad(p, (1, 1, 1, 1))
    p = p[0].permute(1, 2, 0).long()
    return torch.stack([p[dy:dy + gh, dx:dx + gw] for dy in range(3) for dx in range(3)])


def torch_fill_median(vec, valid):
    import torch
    for _ in range(3):
        ok = _neigh(valid[..., None].long(), "zero")
        cnt = ok.sum(dim=0)
        s = (_neigh(vec * valid[..., None], "zero")).sum(dim=0)
        filled = _floor_div(2 * s + cnt, (2 * cnt).clamp(min=1))
        take = ~valid & (cnt[..., 0] > 0)
        vec = torch.where(take[..., None], filled, vec)
        valid = valid | take
    return torch.sort(_neigh(vec, "replicate"), dim=0).values[4]


def _bil(A, qy, qx):
    H, W = A.shape[:2]
    qy, qx = qy.clamp(0, 16 * (H - 1)), qx.clamp(0, 16 * (W - 1))
    iy, ix, fy, fx = qy >> 4, qx >> 4, qy & 15, qx & 15
    iy1, ix1 = (iy + 1).clamp(max=H - 1), (ix + 1).clamp(max=W - 1)
    if A.ndim == 3:
        fy, fx = fy[..., None], fx[..., None]
    return (16 - fy) * ((16 - fx) * A[iy, ix] + fx * A[iy, ix1]) + fy * ((16 - fx) * A[iy1, ix] + fx * A[iy1, ix1])


def torch_advance(P, vec, key):
    import torch
    H, W = key.shape
    gh, gw = vec.shape[:2]
    dev = key.device

    def axis(n, g):
        u = 2 * torch.arange(n, device=dev) - 7
        b0 = u >> 4
        return b0.clamp(0, g - 1), (b0 + 1).clamp(0, g - 1), u - 16 * b0
    y0, y1, fy = axis(H, gh)
    x0, x1, fx = axis(W, gw)
    fy, fx = fy[:, None, None], fx[None, :, None]
    top = (16 - fx) * vec[y0][:, x0] + fx * vec[y0][:, x1]
    bot = (16 - fx) * vec[y1][:, x0] + fx * vec[y1][:, x1]
    V = ((16 - fy) * top + fy * bot + 128) >> 8
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    P = (_bil(P, 16 * yy - V[..., 0], 16 * xx - V[..., 1]) + 128) >> 8
    return P, _bil(key, P[..., 0], P[..., 1])


def torch_propagate(images, mask, levels=LEVELS, search=SEARCH, smooth=SMOOTH):
    """propagate_masks with key frame 0 in torch operators: fp32 [F, H, W]."""
    import torch
    F, H, W = images.shape[:3]
    key = (mask >= 0.5).long()
    Y = torch_luma(images)
    yy, xx = torch.meshgrid(torch.arange(H, device=images.device), torch.arange(W, device=images.device), indexing="ij")
    P, bits = torch.stack([16 * yy, 16 * xx], dim=-1), key
    out = [key.float()]
    src = _pyr(Y[0], levels, True)
    for t in range(1, F):
        tgt, mp, parent = _pyr(Y[t], levels, True), _pyr(bits, levels, False), None
        for lv in range(levels - 1, -1, -1):
            parent = torch_fill_median(*torch_match(src[lv], tgt[lv], mp[lv], parent, search, smooth, lv == 0))
        P, c = torch_advance(P, parent, key)
        out.append(c.float() / 256.0)
        bits, src = (c >= 128).long(), tgt
    return torch.stack(out)


# ---- measurements ------------------------------------------------------------------------------------------------------------------------
def stage_times(job, reps):
    """Every entry alone on the first step's buffers: ms per call, and its count in a whole call."""
    import torch
    from lanpaint_amd import _cabi, propagate
    F, H, W = job["shape"]
    med = fb.median
    out = {}
    out["luma_all_frames"] = med([fb.events(lambda: propagate.luma_pyramids(job["images"], LEVELS)) for _ in range(3)])
    pyr = propagate.luma_pyramids(job["images"][:2], LEVELS)
    out["key_mask"] = fb.events(lambda: propagate.key_mask(job["mask"], LEVELS), reps)
    mpyr, _ = propagate.key_mask(job["mask"], LEVELS)
    step = propagate.Step(H, W, LEVELS, SEARCH, SMOOTH, job["images"].device)
    step.field_of(pyr[0], pyr[1], mpyr)
    torch.cuda.synchronize()
    for lv in range(LEVELS - 1, -1, -1):
        parent = None if lv == LEVELS - 1 else step.field[lv + 1]
        out[f"match_level{lv}"] = fb.events(lambda: propagate.match_level(pyr[0], pyr[1], mpyr, H, W, LEVELS, lv, SEARCH, SMOOTH, parent,
                                                                          step.raw[lv], step.valid[lv]), reps)
        out[f"fill_level{lv}"] = fb.events(lambda: propagate.fill_median(step.raw[lv], step.valid[lv], step.field[lv]), reps)
    key_bits = propagate.level_view(mpyr, H, W, 0)[0]
    o = torch.empty((H, W), dtype=torch.float32, device=key_bits.device)
    out["advance"] = fb.events(lambda: propagate.advance(step.field[0], step.pos[1], key_bits, LEVELS, step.pos[0], o, step.mpyr[0]), reps)
    per_step = sum(v for k, v in out.items() if k.startswith(("match", "fill", "advance")))
    chunks = -(-F * (_cabi.prop_pyramid_ws_bytes(1, H, W, LEVELS)) // propagate.WS_CAP_BYTES)
    return out, per_step, out["luma_all_frames"] + out["key_mask"] + (F - 1) * per_step, chunks


def measure(job, iters, warmup, torch_frames, reps):
    from lanpaint_amd import propagate
    F, H, W = job["shape"]
    call = lambda: propagate.propagate_masks(job["images"], job["mask"], 0, LEVELS, SEARCH, SMOOTH)    # noqa: E731
    names = fb.count_launches(call)
    got = call()
    inter = ((got[-1] >= 0.5) & job["truth"]).sum().item()
    union = ((got[-1] >= 0.5) | job["truth"]).sum().item()
    again = fb.differing(call(), got)
    n = min(torch_frames, F)
    eager = torch_propagate(job["images"][:n], job["mask"])
    differing = fb.differing(eager, propagate.propagate_masks(job["images"][:n], job["mask"], 0, LEVELS, SEARCH, SMOOTH))
    del eager
    fb.untimed(call, warmup)
    s = fb.series([("wall", call, fb.wall), ("events", call),
                   ("torch", lambda: torch_propagate(job["images"][:n], job["mask"]), fb.wall),
                   ("small", lambda: propagate.propagate_masks(job["images"][:n], job["mask"], 0, LEVELS, SEARCH, SMOOTH), fb.wall)], iters, 0)
    walls, evs, torch_ms, small_ms = s["wall"], s["events"], s["torch"], s["small"]
    stages, per_step, busy, chunks = stage_times(job, reps)
    med = fb.median
    whole = med(walls)
    per = {k: names.count(k) for k in sorted(set(names))}
    return {"case": job["case"], "frames_height_width": [F, H, W], "levels": LEVELS, "search": SEARCH, "smooth": SMOOTH,
            "whole_wall_ms": round(whole, 3), "whole_wall_min_max_ms": fb.summary(walls, 3)[1],
            "whole_events_ms": round(med(evs), 3), "ms_per_frame": round(whole / F, 4),
            "launches_per_call": len(names), "launches_by_entry": per,
            "launches_per_step": (per.get("lp_prop_match", 0) + per.get("lp_prop_fill", 0) + per.get("lp_prop_advance", 0)) // max(F - 1, 1),
            "dependent_steps": F - 1, "luma_chunks": chunks,
            "stage_ms": {k: round(v, 5) for k, v in stages.items()}, "stage_reps": reps, "step_ms_from_stages": round(per_step, 4),
            "busy_ms_from_stages": round(busy, 3), "launch_gap_share_estimate": round(max(0.0, 1 - busy / whole), 3),
            "iou_last_frame": round(inter / max(union, 1), 4), "elements_differing_between_two_calls": again,
            "torch_frames": n, "torch_ms": round(med(torch_ms), 3), "module_ms_same_frames": round(med(small_ms), 3),
            "torch_over_module": round(med(torch_ms) / med(small_ms), 2), "elements_differing_from_torch": differing}


def main():
    ap = fb.parser(CASES, ("whole",), iters=5, warmup=1)
    ap.add_argument("--reps", type=int, default=50, help="back-to-back calls per stage timing")
    ap.add_argument("--torch-frames", type=int, default=4)
    a = ap.parse_args()
    dev = fb.device()
    import torch
    from lanpaint_amd import propagate
    results = []
    for case in ((a.case,) if a.case else tuple(CASES)):
        job = make_job(case, dev)
        if a.job:
            fb.untimed(lambda: propagate.propagate_masks(job["images"], job["mask"], 0, LEVELS, SEARCH, SMOOTH), a.warmup + a.iters)
        else:
            results.append(measure(job, a.iters, a.warmup, a.torch_frames, a.reps))
        del job
        torch.cuda.empty_cache()
    if not a.job:
        fb.emit("mask_propagate", a, results)


if __name__ == "__main__":
    main()
