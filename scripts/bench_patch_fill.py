#!/usr/bin/env python3
"""Patch fill benchmark (lanpaint_amd.fill.fill_masked_patch on the HIP device): one JSON line.

Two cases, everything already on the device, a textured image (a random 24 x 32 tile repeated, plus 2 % noise):

    frame   1 x 1024 x 1024 x 3 under a 256 x 256 hole
    clip    81 x 720 x 1280 x 3 under the benchmark's disc (radius 150, drifting across the frame)

    patch   fill_masked_patch at its defaults (radius 3, levels AUTO, iters 4, seed 0): lp_mask_fill's patch form
    smooth  fill_masked on the same tensors, in the same process: what the patch form costs over the push-pull fill
    eager   the patch rule composed from torch operators on the same device -- the vectorised Jacobi form of
            tests/patch_fill_ref.py over all targets of the batch at once, Philox4x32-10 in int64 -- behind the same HIP pre-fill.
            Its output is compared with the kernel's: the count of differing elements is reported (0 expected).
    parent  with --parent-lib: lp_mask_fill with reserved0 = 0 called directly in this build's library and in the given one (the
            parent revision's), alternating, on the same tensors: the push-pull path is untouched, so the two medians must sit
            inside the spread of either one's two series.

    python scripts/bench_patch_fill.py [--iters 10] [--warmup 2] [--case frame] [--parent-lib PATH] [--no-eager]
    python scripts/bench_patch_fill.py --job patch --case frame --iters 3      # the body of a rocprofv3 --kernel-trace --stats run

Time: featurebench.events per call; every iteration runs patch, smooth, patch, smooth.
"""
from __future__ import annotations

import ctypes

import featurebench as fb

CASES = ("frame", "clip")
RADIUS, ITERS, SEED = 3, 4, 0
M32 = 0xFFFFFFFF


def make_job(case, dev):
    import torch
    g = torch.Generator(device="cpu").manual_seed(0)
    frames, H, W = (1, 1024, 1024) if case == "frame" else (81, 720, 1280)
    tile = 0.1 + 0.8 * torch.rand(24, 32, 3, generator=g)
    image = tile.repeat(-(-H // 24), -(-W // 32), 1)[:H, :W].expand(frames, -1, -1, -1)
    image = (image + 0.02 * torch.rand(frames, H, W, 3, generator=g)).contiguous()
    mask = torch.zeros(frames, H, W)
    if case == "frame":
        mask[:, 384:640, 384:640] = 1.0
    else:
        yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        for f in range(frames):
            cx = 300 + (W - 600) * f // (frames - 1)
            mask[f] = ((yy - H // 2) ** 2 + (xx - cx) ** 2 < 150 * 150).float()
    return {"case": case, "image": image.to(dev), "mask": mask.to(dev)}


def patch_job(j):
    from lanpaint_amd import fill
    return fill.fill_masked_patch(j["image"], j["mask"], RADIUS, fill.AUTO, ITERS, SEED)


def smooth_job(j):
    from lanpaint_amd import fill
    return fill.fill_masked(j["image"], j["mask"])


# ---- the rule in torch operators ----------------------------------------------------------------------------------------------------
def _philox(ctr, sub, seed):
    """Philox4x32-10 on int64 tensors holding 32-bit words (a 32 x 32 product wraps to the right low 64 bits): words 0 and 1."""
    c0, c1, c2, c3 = ctr & M32, ctr >> 32, sub & M32, sub >> 32
    k0, k1 = seed & M32, (seed >> 32) & M32
    for _ in range(10):
        p0, p1 = c0 * 0xD2511F53, c2 * 0xCD9E8D57
        c0, c1, c2, c3 = ((p1 >> 32) & M32) ^ c1 ^ k0, p1 & M32, ((p0 >> 32) & M32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1


class _Level:
    def __init__(self, I, hole, r):
        import torch
        import torch.nn.functional as F
        self.I, self.hole, self.r = I, hole, r
        B, self.h, self.w, _ = I.shape
        near = F.max_pool2d(hole[:, None].float(), 2 * r + 1, 1, r)[:, 0] > 0
        y, x = torch.meshgrid(torch.arange(self.h, device=I.device), torch.arange(self.w, device=I.device), indexing="ij")
        whole = (y - r >= 0) & (y + r < self.h) & (x - r >= 0) & (x + r < self.w)
        self.target, self.source = near, whole[None] & ~near
        self.T = I.clone()
        self.tb, self.ty, self.tx = torch.nonzero(near, as_tuple=True)
        self.qb, self.qy, self.qx = torch.nonzero(hole, as_tuple=True)

    def distance(self, sy, sx, ok):
        import torch
        r, h, w = self.r, self.h, self.w
        sy, sx = torch.where(ok, sy, r), torch.where(ok, sx, r)
        D = torch.zeros_like(sy)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                ty, tx = self.ty + dy, self.tx + dx
                inside = (ty >= 0) & (ty < h) & (tx >= 0) & (tx < w)
                a = self.T[self.tb, ty.clamp(0, h - 1), tx.clamp(0, w - 1)]
                b = self.I[self.tb, (sy + dy).clamp(0, h - 1), (sx + dx).clamp(0, w - 1)]
                D += torch.where(inside, (a - b).abs().sum(1), 0)
        return torch.where(ok, D, 1 << 40)

    def search(self, nnf, level, rnd, seed):
        import torch
        h, w, tb, py, px = self.h, self.w, self.tb, self.ty, self.tx
        best = [torch.full_like(py, 1 << 40), torch.full_like(py, -1), torch.full_like(py, -1)]

        def consider(cy, cx, ok):
            ok = ok & (cy >= 0) & (cy < h) & (cx >= 0) & (cx < w)
            ok = ok & self.source[tb, cy.clamp(0, h - 1), cx.clamp(0, w - 1)]
            D = self.distance(cy, cx, ok)
            better = ok & ((D < best[0]) | ((D == best[0]) & ((cy < best[1]) | ((cy == best[1]) & (cx < best[2])))))
            best[0], best[1], best[2] = torch.where(better, D, best[0]), torch.where(better, cy, best[1]), torch.where(better, cx, best[2])

        own = nnf[tb, py, px]
        consider(own[:, 0], own[:, 1], own[:, 0] >= 0)
        for step in (1, 4):
            for ey, ex in ((0, -1), (-1, 0), (0, 1), (1, 0)):
                ny, nx = py + step * ey, px + step * ex
                inside = (ny >= 0) & (ny < h) & (nx >= 0) & (nx < w)
                cy_, cx_ = ny.clamp(0, h - 1), nx.clamp(0, w - 1)
                e = nnf[tb, cy_, cx_]
                consider(e[:, 0] - step * ey, e[:, 1] - step * ex, inside & self.target[tb, cy_, cx_] & (e[:, 0] >= 0))
        j = 0
        while (max(h, w) >> j) >= 1:
            R = max(h, w) >> j
            valid = best[1] >= 0
            cy, cx = torch.where(valid, best[1], py), torch.where(valid, best[2], px)
            sub = torch.full_like(py, (level << 40) | (rnd << 32) | j)
            w0, w1 = _philox(py * 65536 + px, sub, torch.full_like(py, seed))
            consider(cy + ((w0 * (2 * R + 1)) >> 32) - R, cx + ((w1 * (2 * R + 1)) >> 32) - R, torch.ones_like(valid))
            j += 1
        out = torch.full_like(nnf, -1)
        out[tb, py, px] = torch.stack(best[1:], 1)
        return out

    def vote(self, nnf):
        import torch
        r, h, w, qb, qy, qx = self.r, self.h, self.w, self.qb, self.qy, self.qx
        s = torch.zeros((len(qy), self.I.shape[3]), dtype=torch.int64, device=qy.device)
        n = torch.zeros_like(qy)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                y, x = qy - dy, qx - dx
                e = nnf[qb, y.clamp(0, h - 1), x.clamp(0, w - 1)]
                ok = (y >= 0) & (y < h) & (x >= 0) & (x < w) & (e[:, 0] >= 0)
                val = self.I[qb, (e[:, 0] + dy).clamp(0, h - 1), (e[:, 1] + dx).clamp(0, w - 1)]
                s += torch.where(ok[:, None], val, 0)
                n += ok
        got = n > 0
        nn = torch.where(got, n, 1)[:, None]
        self.T[qb[got], qy[got], qx[got]] = ((s + nn // 2) // nn)[got]
        voted = torch.zeros_like(self.hole)
        voted[qb[got], qy[got], qx[got]] = True
        return voted

    def field_from(self, coarse):
        import torch
        h, w = self.h, self.w
        y, x = torch.meshgrid(torch.arange(h, device=coarse.device), torch.arange(w, device=coarse.device), indexing="ij")
        up = coarse[:, y >> 1, x >> 1]
        sy, sx = 2 * up[..., 0] + (y & 1), 2 * up[..., 1] + (x & 1)
        ok = self.target & (up[..., 0] >= 0) & (sy < h) & (sx < w)
        b = torch.arange(coarse.shape[0], device=coarse.device)[:, None, None].expand_as(sy)
        ok = ok & self.source[b, sy.clamp(0, h - 1), sx.clamp(0, w - 1)]
        return torch.where(ok[..., None], torch.stack((sy, sx), -1), -1)


def eager_patch(pp, image, mask, r, levels, iters, seed):
    """The patch rule behind the pre-fill `pp`, in torch operators: image [B, H, W, C], mask [Bm, H, W]."""
    import torch
    import torch.nn.functional as F
    B = image.shape[0]
    hole = (mask > 0.5).expand(B, -1, -1)
    t = torch.floor(pp * 255.0 + 0.5)                                  # (torch does not fuse the product and the sum)
    I = torch.where(torch.isnan(t), 0.0, t).clamp(0, 255).long()
    pyramid = [_Level(I, hole, r)]
    for _ in range(1, levels):
        h, w = I.shape[1:3]
        Ip = F.pad(I, (0, 0, 0, w % 2, 0, h % 2))
        n = F.pad(torch.ones(1, h, w, dtype=torch.int64, device=I.device), (0, w % 2, 0, h % 2))
        hp = F.pad(hole.to(torch.uint8), (0, w % 2, 0, h % 2)) > 0
        s = sum(Ip[:, dy::2, dx::2] for dy in (0, 1) for dx in (0, 1))
        cnt = sum(n[:, dy::2, dx::2] for dy in (0, 1) for dx in (0, 1))[..., None]
        I, hole = (s + cnt // 2) // cnt, hp[:, 0::2, 0::2] | hp[:, 0::2, 1::2] | hp[:, 1::2, 0::2] | hp[:, 1::2, 1::2]
        pyramid.append(_Level(I, hole, r))
    nnf = voted = None
    for l in range(levels - 1, -1, -1):
        g = pyramid[l]
        if nnf is None:
            nnf = torch.full((B, g.h, g.w, 2), -1, dtype=torch.int64, device=I.device)
        else:
            nnf = g.field_from(nnf)
            g.vote(nnf)
        for rnd in range(iters):
            nnf = g.search(nnf, l, rnd, seed)
            voted = g.vote(nnf)
    # (a 0-dim device tensor as divisor: by a Python number torch multiplies by the reciprocal, which is not the IEEE quotient)
    out = torch.where(voted[..., None], pyramid[0].T.float() / torch.full((), 255.0, device=pp.device), pp)
    return torch.where((mask > 0.5)[..., None], out, image)


def eager_job(j):
    from lanpaint_amd import fill
    h, w = j["image"].shape[1:3]
    return eager_patch(fill.fill_masked(j["image"], j["mask"]), j["image"], j["mask"], RADIUS, fill.patch_levels(h, w, RADIUS), ITERS, SEED)


# ---- the push-pull entry in two libraries ---------------------------------------------------------------------------------------------
def parent_series(job, parent_lib, iters, warmup):
    """Device times of lp_mask_fill (reserved0 = 0) in this build's library and in `parent_lib`, alternating: four series."""
    import torch
    from lanpaint_amd import _cabi
    from lanpaint_amd._util import raw_stream
    img, mask = job["image"], job["mask"]
    b, h, w, c = img.shape
    dev = img.device
    libs = {"this": _cabi.load(), "parent": _cabi.load(parent_lib)}
    ws = torch.empty(_cabi.fill_ws_bytes(b, h, w, c), dtype=torch.uint8, device=dev)
    out = torch.empty_like(img)
    d = _cabi.LpFillDesc(b, h, w, c, mask.shape[0], 0, img.data_ptr(), mask.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel())

    def entry(lib):
        rc = lib.lp_mask_fill(ctypes.byref(d), raw_stream(dev))
        assert rc == 0, rc
    ours, theirs = (lambda lib=lib: entry(lib) for lib in (libs["this"], libs["parent"]))
    rec = fb.series([("this_a", ours), ("parent_a", theirs), ("this_b", ours), ("parent_b", theirs)], iters, warmup)
    med = fb.median
    this, parent = med(rec["this_a"] + rec["this_b"]), med(rec["parent_a"] + rec["parent_b"])
    return {"this_ms": round(this, 4), "parent_ms": round(parent, 4), "this_over_parent": round(this / parent, 4),
            "this_spread": fb.spread(rec["this_a"], rec["this_b"]),
            "parent_spread": fb.spread(rec["parent_a"], rec["parent_b"]),
            "this_min_max_ms": fb.summary(rec["this_a"] + rec["this_b"])[1],
            "parent_min_max_ms": fb.summary(rec["parent_a"] + rec["parent_b"])[1]}


def measure(case, dev, iters, warmup, eager, parent_lib):
    import torch
    from lanpaint_amd import fill
    job = make_job(case, dev)
    run_patch, run_smooth, run_eager = (lambda f=f: f(job) for f in (patch_job, smooth_job, eager_job))
    rec = fb.series([("patch_a", run_patch), ("smooth_a", run_smooth), ("patch_b", run_patch), ("smooth_b", run_smooth)], iters, warmup)
    med = fb.median
    patch, smooth = med(rec["patch_a"] + rec["patch_b"]), med(rec["smooth_a"] + rec["smooth_b"])
    got = patch_job(job)
    hole = job["mask"] > 0.5
    res = {"case": case, "image": list(job["image"].shape), "levels": fill.patch_levels(*job["image"].shape[1:3], RADIUS),
           "hole_pixels": int(hole.sum()),
           "patch_ms": round(patch, 3), "smooth_ms": round(smooth, 4), "patch_over_smooth": round(patch / smooth, 1),
           "patch_min_max_ms": fb.summary(rec["patch_a"] + rec["patch_b"], 3)[1],
           "patch_spread": fb.spread(rec["patch_a"], rec["patch_b"]),
           "smooth_spread": fb.spread(rec["smooth_a"], rec["smooth_b"]),
           "changed_from_smooth": fb.differing(got, smooth_job(job))}
    if eager:
        times = fb.series([("eager", run_eager)], max(2, iters // 4), 1)["eager"]
        want = eager_job(job)
        res.update({"eager_ms": round(med(times), 2), "eager_over_patch": round(med(times) / patch, 1),
                    "elements_differing_from_eager": fb.differing(got.view(torch.int32), want.view(torch.int32)),
                    "codes_differing_from_eager": fb.differing(torch.floor(got * 255.0 + 0.5), torch.floor(want * 255.0 + 0.5))})
        del want
    if parent_lib:
        res["push_pull_vs_parent"] = parent_series(job, parent_lib, max(iters, 20), warmup)
    return res


def main():
    ap = fb.parser(CASES, ("patch", "smooth", "eager"))
    ap.add_argument("--no-eager", action="store_true", help="leave the torch-operator side out")
    ap.add_argument("--parent-lib", help="another build of liblanpaint_hip.so to time lp_mask_fill's push-pull form against")
    a = ap.parse_args()
    dev = fb.device()
    import torch
    cases = (a.case,) if a.case else CASES
    if a.job:
        fn = {"patch": patch_job, "smooth": smooth_job, "eager": eager_job}[a.job]
        for case in cases:
            job = make_job(case, dev)
            fb.untimed(lambda: fn(job), a.warmup + a.iters)
        return
    results = []
    for case in cases:
        results.append(measure(case, dev, a.iters, a.warmup, not a.no_eager, a.parent_lib))
        torch.cuda.empty_cache()
    fb.emit("patch_fill", a, results, radius=RADIUS, patch_iters=ITERS)


if __name__ == "__main__":
    main()
