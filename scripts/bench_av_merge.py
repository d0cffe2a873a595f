#!/usr/bin/env python3
"""AV decode audio merge benchmark (lanpaint_amd.audio.merge_audio_with_mask -> lp_audio_merge): one JSON line.

Shapes: stereo 48 kHz with a 25 fps hard 0/1 mask of several intervals, crossfade 0.02 s (960 samples):
    10s   n = 480 000, 250 mask frames
    60s   n = 2 880 000, 1 500 mask frames

For each shape, three timings of the same merge:
    hip         merge_audio_with_mask on device waveforms with the host mask a ComfyUI node hands over (its copy included)
    torch_dev   the reference's torch sequence (nodes.py:1091-1136: interpolate nearest-exact, replicate pad, conv1d, lerp)
                on the device, mask on the device
    torch_host  the same sequence on host tensors (where the reference runs it in a ComfyUI workflow)

    python scripts/bench_av_merge.py [--iters 30] [--warmup 5] [--host-iters 3] [--kernels 10s=A.db 60s=B.db]
    python scripts/bench_av_merge.py --shape 10s --iters 20      # the body of a rocprofv3 --kernel-trace run

Time: featurebench.wall per call, median over --iters after --warmup (torch_host without the device synchronise).  Per-kernel
times come from a SEPARATE rocprofv3 --kernel-trace --stats run per shape (--kernels reads its results .db / CSV); the merge
kernel's bytes (two fp32 reads and one write per sample and channel) over its median time are reported against 6.3 TB/s.
"""
from __future__ import annotations

import featurebench as fb

HBM_ACHIEVABLE = 6.3e12
SR, FPS, CROSSFADE, CHANNELS = 48000, 25, 0.02, 2
SHAPES = {"10s": 10, "60s": 60}


def inputs(seconds, dev):
    import torch
    n, fm = seconds * SR, seconds * FPS
    g = torch.Generator(device="cpu").manual_seed(seconds)
    orig = (0.3 * torch.randn(1, CHANNELS, n, generator=g)).to(dev)
    inp = (0.3 * torch.randn(1, CHANNELS, n, generator=g)).to(dev)
    mask = torch.zeros(fm)
    for k in range(0, fm, 100):                  # 2 s of every 4 regenerated, plus single-frame blips
        mask[k + 10:k + 60] = 1.0
        mask[min(k + 80, fm - 1)] = 1.0
    return orig, inp, mask


def torch_sequence(orig, inp, am, crossfade, sr):
    import torch
    F = torch.nn.functional
    n = orig.shape[-1]
    w = F.interpolate(am[None, None], size=(n,), mode="nearest-exact")[0, 0]
    cf = max(1, int(round(crossfade * sr)))
    k = torch.ones(1, 1, cf, device=orig.device) / cf
    w = F.conv1d(F.pad(w[None, None], (cf // 2, cf - 1 - cf // 2), mode="replicate"), k)[0, 0][..., :n]
    return orig * (1 - w[None, None]) + inp * w[None, None]


def wall_stats(fn, iters, warmup, sync=fb.synchronize):
    ms, (low, high) = fb.summary(fb.series([("wall", fn)], iters, warmup, timer=lambda f: fb.wall(f, sync=sync), sync=sync)["wall"])
    return {"ms_median": ms, "ms_min": low, "ms_max": high, "iters": iters}


def kernel_stats(path):
    from rocprof_summary import rows_from_csv, rows_from_db
    rows = rows_from_db(path) if path.endswith(".db") else rows_from_csv(path)
    per = {}
    for name, start, end, *_ in rows:
        for k in ("plan", "merge"):
            if f"lp_audio_{k}_kernel" in name:
                per.setdefault(k, []).append((end - start) * 1e-3)
    return {k: {"calls": len(v), "mean_us": round(sum(v) / len(v), 2), "median_us": round(fb.median(v), 2)}
            for k, v in per.items()}


def run_hip(seconds, iters, warmup):
    from lanpaint_amd import audio
    orig, inp, mask = inputs(seconds, fb.device())
    return wall_stats(lambda: audio.merge_audio_with_mask(orig, inp, mask, CROSSFADE, SR, SR), iters, warmup)


def main():
    ap = fb.parser(iters=30, warmup=5)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--shape", choices=sorted(SHAPES))
    ap.add_argument("--kernels", nargs="*", default=[], help="SHAPE=rocprofv3 results .db or kernel-trace .csv")
    args = ap.parse_args()
    dev = fb.device()
    import torch
    if args.shape:
        run_hip(SHAPES[args.shape], args.iters, args.warmup)
        return
    from lanpaint_amd import audio
    profiles = dict(kv.split("=", 1) for kv in args.kernels)
    shapes = {}
    for name in sorted(SHAPES, key=SHAPES.get):
        seconds = SHAPES[name]
        orig, inp, mask = inputs(seconds, dev)
        n = orig.shape[-1]
        got = audio.merge_audio_with_mask(orig, inp, mask, CROSSFADE, SR, SR)
        want = torch_sequence(orig, inp, mask.to(dev), CROSSFADE, SR)
        rec = {"n": n, "mask_frames": int(mask.numel()), "bytes": 3 * 4 * CHANNELS * n,
               "max_abs_diff_vs_torch_dev": float((got - want).abs().max()),
               "hip": run_hip(seconds, args.iters, args.warmup),
               "torch_dev": wall_stats(lambda: torch_sequence(orig, inp, mask.to(dev), CROSSFADE, SR), args.iters, args.warmup)}
        o_h, i_h = orig.cpu(), inp.cpu()
        rec["torch_host"] = wall_stats(lambda: torch_sequence(o_h, i_h, mask, CROSSFADE, SR), args.host_iters, 1, sync=lambda: None)
        if name in profiles:
            ks = kernel_stats(profiles[name])
            rec["kernels"] = ks
            if "merge" in ks:
                rec["merge_kernel_hbm_frac"] = round(rec["bytes"] / (ks["merge"]["median_us"] * 1e-6) / HBM_ACHIEVABLE, 4)
        else:
            rec["kernels"] = "not measured"
        shapes[name] = rec
        del orig, inp, got, want
        torch.cuda.empty_cache()
    fb.emit("av_audio_merge", None, sample_rate=SR, channels=CHANNELS, crossfade_s=CROSSFADE, torch_threads=torch.get_num_threads(),
            shapes=shapes)


if __name__ == "__main__":
    main()
