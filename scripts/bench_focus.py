#!/usr/bin/env python3
"""Focus match benchmark (lanpaint_amd.focus on the HIP device): one JSON line.

Two cases, everything already on the device: grey blocks of 8 x 8 pixels, soft (a Gaussian of sigma 1.5) everywhere but under the
disc, where they are sharp -- the inpaint that is too crisp for its shot.  The reference is the soft picture.

    frame  match_focus of 1 x 1024 x 1024 x 3 through a soft disc of radius 150
    clip   the same for 81 x 720 x 1280 x 3, the disc drifting across the frame, the clip measured as one (per_frame off)

    hip    lanpaint_amd.focus: lp_multiband_blend with LP_MULTIBAND_FOCUS (flags, stats, fit, rows, columns: five launches)
    torch  the same rule restated in torch operators on the same device (integer tensors up to the fit, fp64 for the fit, fp32
           slices times taps for the blur, one operator per rounding; it reads K back to size its loops).  It has to agree in
           every element: the count of differing elements is printed, also for K and both variances.
    clone  torch.clone of the case's image: the copy rate this process reaches on these very tensors, in the same run.
    parent with --parent-lib: lp_multiband_blend at levels = 5 called directly in this build's library and in the given one (the
           parent revision's), alternating, on the same tensors: the entry gained a branch on the sign of `levels`, so the two
           medians must sit inside each other's spread.

    python scripts/bench_focus.py [--iters 10] [--warmup 2] [--case frame] [--parent-lib PATH]
    python scripts/bench_focus.py --job hip --case frame --iters 5      # the body of a rocprofv3 --kernel-trace --stats run

Time: featurebench.events per call; every iteration runs hip, torch, hip, torch, clone (the torch side's iterations are capped: it is
slow).  Bytes: what the rule has to move at the least -- image, reference and mask read once, the result written once -- over the
time, and that rate over the clone's (one read, one write).
"""
from __future__ import annotations

import ctypes
import math

import featurebench as fb

CASES = {"frame": (1, 1024, 1024, 3), "clip": (81, 720, 1280, 3)}
RADIUS, EDGE, RING, STRENGTH = 150, 8, 2, 1.0
TORCH_ITERS = 3
B8 = (1, 8, 28, 56, 70, 56, 28, 8, 1)


def _gauss(x, sigma):
    """[B, H, W, C] through a Gaussian, replicate-padded: the scene's softness, not part of what is measured"""
    import torch
    import torch.nn.functional as F
    r = int(math.ceil(4 * sigma))
    k = torch.exp(-torch.arange(-r, r + 1, dtype=torch.float32, device=x.device) ** 2 / (2 * sigma * sigma))
    k = k / k.sum()
    c = x.shape[3]
    x = x.permute(0, 3, 1, 2)
    x = F.conv2d(F.pad(x, (0, 0, r, r), mode="replicate"), k.view(1, 1, -1, 1).expand(c, 1, -1, 1), groups=c)
    x = F.conv2d(F.pad(x, (r, r, 0, 0), mode="replicate"), k.view(1, 1, 1, -1).expand(c, 1, 1, -1), groups=c)
    return x.permute(0, 2, 3, 1).contiguous()


def make_job(case, dev):
    import torch
    B, H, W, C = CASES[case]
    g = torch.Generator(device="cpu").manual_seed(0)
    grey = torch.rand(B, -(-H // 8), -(-W // 8), C, generator=g).to(dev)
    sharp = grey.repeat_interleave(8, 1).repeat_interleave(8, 2)[:, :H, :W].contiguous()
    soft = torch.cat([_gauss(sharp[s:s + 9], 1.5) for s in range(0, B, 9)])
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    mask = torch.zeros(B, H, W)
    for f in range(B):
        cx = W // 2 if B == 1 else 300 + (W - 600) * f // (B - 1)
        dist = ((yy - H // 2) ** 2 + (xx - cx) ** 2).float().sqrt()
        mask[f] = ((RADIUS - dist) / 8.0 + 0.5).clamp(0.0, 1.0)          # a disc with a soft rim of 8 pixels
    mask = mask.to(dev)
    image = torch.where(mask.unsqueeze(-1) > 0, sharp, soft).contiguous()
    return {"case": case, "image": image, "reference": soft, "mask": mask}


def required_bytes(case):
    B, H, W, C = CASES[case]
    image, mask = B * H * W * C * 4, B * H * W * 4
    return {"job": 3 * image + mask, "clone": 2 * image}


def hip_job(j):
    from lanpaint_amd import focus
    return focus.focus_report(j["image"], j["mask"], j["reference"], STRENGTH, EDGE, RING, False)


def clone(j):
    return j["image"].clone()


# ---- the rule in torch operators ---------------------------------------------------------------------------------------------------------
def _luma(img):
    import torch
    t = torch.where(img > 0, img.clamp(max=1.0), torch.zeros_like(img))
    c = (t * 255.0 + 0.5).to(torch.int64)
    return (77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8 if img.shape[-1] >= 3 else c[..., 0]


def _sep(y, k):
    n = len(k)
    h = sum(k[i] * y[:, :, i:y.shape[2] - n + 1 + i] for i in range(n))
    return sum(k[i] * h[:, i:h.shape[1] - n + 1 + i] for i in range(n))


def _grad2(p):
    gx, gy = p[:, 1:-1, 2:] - p[:, 1:-1, :-2], p[:, 2:, 1:-1] - p[:, :-2, 1:-1]
    return gx * gx + gy * gy


def _stats(img, region, thr):
    import torch
    y = _luma(img)
    ga, gb = _grad2(_sep(y[:, 3:-3, 3:-3], (1, 2, 1))), _grad2(_sep(y, B8))
    use = region & (gb >= thr)
    zero = torch.zeros_like(ga)
    return use.sum(), torch.where(use, ga, zero).sum(), torch.where(use, gb >> 16, zero).sum()


def _variance(n, sa, sb):
    import torch
    r = (sa.double() / 256.0) / (sb.double() / 65536.0)
    q = r * r
    return torch.where(n < 64, -1.0, torch.where(q > 1.0, (2.0 - 0.5 * q) / (q - 1.0), 16.0))


def torch_focus(image, reference, mask, strength16, edge, ring):
    """The pooled rule of include/lanpaint_hip.h in torch operators: images [B, H, W, C], mask [B, H, W] -> (out, var pair, K)."""
    import torch
    import torch.nn.functional as F
    B, H, W, C = image.shape
    masked = (mask > 0.5).float().unsqueeze(1)
    count = F.avg_pool2d(masked, 11, stride=1, divisor_override=1)[:, 0]                       # exact: at most 121 ones
    marked = F.max_pool2d(masked, 32, stride=32, ceil_mode=True)
    near = F.max_pool2d(marked, 2 * ring + 1, stride=1, padding=ring)
    near = near.repeat_interleave(32, 2).repeat_interleave(32, 3)[:, 0, 5:H - 5, 5:W - 5] > 0
    thr = (edge * 2 * 65536) ** 2
    ring_s = _stats(reference, (count == 0) & near, thr)
    in_s = _stats(image, count == 121, thr)
    var_ring, var_inside = _variance(*ring_s), _variance(*in_s)
    d = (var_ring - var_inside).clamp(min=0.0)
    v = ((strength16 / 16.0) * d).clamp(max=16.0)
    K = torch.where((ring_s[0] >= 64) & (in_s[0] >= 64), (v * 32.0 + 0.5).to(torch.int32), 0)
    Kh = int(K.item())
    if Kh == 0:
        return image.clone(), (var_ring, var_inside), K
    k, t = Kh >> 4, Kh & 15
    r = k + (1 if t else 0)
    taps = []
    for i in range(-r, r + 1):
        j = abs(i)
        b0 = math.ldexp(float(math.comb(2 * k, k + j)), -2 * k) if j <= k else 0.0
        b1 = math.ldexp(float(math.comb(2 * k + 2, k + 1 + j)), -2 * k - 2)
        taps.append(torch.tensor(((16 - t) * b0 + t * b1) / 16.0, dtype=torch.float64).float().item())
    x = image
    for axis, n in ((2, W), (1, H)):
        idx = torch.arange(n, device=image.device)
        s = None
        for i, w in zip(range(-r, r + 1), taps):
            term = x.index_select(axis, (idx + i).clamp(0, n - 1)) * w
            s = term if s is None else s + term
        x = s
    m = torch.where(mask > 0, mask.clamp(max=1.0), torch.zeros_like(mask)).unsqueeze(-1)
    return torch.where(m > 0, image + m * (x - image), image), (var_ring, var_inside), K


def torch_job(j):
    return torch_focus(j["image"], j["reference"], j["mask"], int(STRENGTH * 16 + 0.5), EDGE, RING)


# ---- the plain blend in two libraries ----------------------------------------------------------------------------------------------------
def parent_series(job, parent_lib, iters, warmup, levels=5):
    """Device times of lp_multiband_blend (levels >= 0) in this build's library and in `parent_lib`, alternating: four series."""
    import torch
    from lanpaint_amd import _cabi
    from lanpaint_amd._util import raw_stream
    a, b, mask = job["reference"], job["image"], job["mask"]
    B, H, W, C = a.shape
    dev = a.device
    libs = (_cabi.load(), _cabi.load(parent_lib))
    ws = torch.empty(_cabi.multiband_ws_bytes(B, H, W, C, levels), dtype=torch.uint8, device=dev)
    out = torch.empty_like(a)
    d = _cabi.LpMultibandDesc(B, H, W, C, mask.shape[0], levels, a.data_ptr(), b.data_ptr(), mask.data_ptr(), out.data_ptr(),
                              ws.data_ptr(), ws.numel())

    def entry(lib):
        rc = lib.lp_multiband_blend(ctypes.byref(d), raw_stream(dev))
        assert rc == 0, rc
    ours, theirs = (lambda lib=lib: entry(lib) for lib in libs)
    rec = fb.series([("this_a", ours), ("parent_a", theirs), ("this_b", ours), ("parent_b", theirs)], iters, warmup)
    med = fb.median
    this, parent = med(rec["this_a"] + rec["this_b"]), med(rec["parent_a"] + rec["parent_b"])
    return {"levels": levels, "this_ms": round(this, 4), "parent_ms": round(parent, 4), "this_over_parent": round(this / parent, 4),
            "this_spread": fb.spread(rec["this_a"], rec["this_b"]), "parent_spread": fb.spread(rec["parent_a"], rec["parent_b"]),
            "this_min_max_ms": fb.summary(rec["this_a"] + rec["this_b"])[1],
            "parent_min_max_ms": fb.summary(rec["parent_a"] + rec["parent_b"])[1]}


def run(job, iters, warmup, only=None):
    hip, eager, copy = (lambda f=f: f(job) for f in (hip_job, torch_job, clone))
    if only:
        return fb.series([(only + "_a", hip if only == "hip" else eager)], iters, warmup)
    s = fb.series([("hip_a", hip), ("hip_b", hip), ("clone", copy)], iters, warmup)
    s.update(fb.series([("torch_a", eager), ("torch_b", eager)], min(iters, TORCH_ITERS), 1))
    return s


def measure(case, dev, iters, warmup, parent_lib=None):
    import torch
    job = make_job(case, dev)
    rep, (out, var, K) = hip_job(job), torch_job(job)
    differ = {"image": fb.differing(rep["image"], out), "K": fb.differing(rep["K"], K.expand_as(rep["K"])),
              "var": fb.differing((rep["var_ring"], rep["var_inside"]), tuple(v.expand_as(rep["var_ring"]) for v in var))}
    changed = fb.differing(rep["image"], job["image"])
    fitted = {"K": int(rep["K"][0]), "sigma": round(math.sqrt(int(rep["K"][0]) / 32.0), 3), "var_ring": round(float(rep["var_ring"][0]), 4),
              "var_inside": round(float(rep["var_inside"][0]), 4)}
    del rep, out
    torch.cuda.empty_cache()
    s = run(job, iters, warmup)
    med = fb.median
    need = required_bytes(case)
    hip, eager = med(s["hip_a"] + s["hip_b"]), med(s["torch_a"] + s["torch_b"])
    clone_tbs = need["clone"] / (med(s["clone"]) * 1e-3) / 1e12
    rate = need["job"] / (hip * 1e-3) / 1e12
    more = {"multiband_vs_parent": parent_series(job, parent_lib, max(iters, 20), warmup)} if parent_lib else {}
    return {**more, "case": case, "image": list(job["image"].shape), "fitted": fitted, "elements_changed": changed,
            "elements_differing_hip_torch": differ, "hip_ms": round(hip, 4), "torch_ms": round(eager, 4),
            "torch_over_hip": round(eager / hip, 2), "hip_min_max_ms": fb.summary(s["hip_a"] + s["hip_b"])[1],
            "hip_spread": fb.spread(s["hip_a"], s["hip_b"]), "torch_spread": fb.spread(s["torch_a"], s["torch_b"]),
            "clone_ms": round(med(s["clone"]), 4), "hip_over_clone": round(hip / med(s["clone"]), 2),
            "clone_tb_per_s": round(clone_tbs, 3), "required_bytes": need, "required_tb_per_s": round(rate, 3),
            "fraction_of_clone_rate": round(rate / clone_tbs, 3)}


def main():
    ap = fb.parser(CASES, ("hip", "torch"), iters=10, warmup=2)
    ap.add_argument("--parent-lib", help="another build of liblanpaint_hip.so to time lp_multiband_blend's plain form against")
    a = ap.parse_args()
    dev = fb.device()
    import torch
    cases = (a.case,) if a.case else tuple(CASES)
    if a.job:
        for case in cases:
            run(make_job(case, dev), a.iters, a.warmup, only=a.job)
        return
    results = []
    for case in cases:
        results.append(measure(case, dev, a.iters, a.warmup, a.parent_lib))
        torch.cuda.empty_cache()
    fb.emit("focus_match", a, results, strength=STRENGTH, edge=EDGE, ring=RING,
            torch_agrees_in_every_element=all(sum(r["elements_differing_hip_torch"].values()) == 0 for r in results))


if __name__ == "__main__":
    main()
