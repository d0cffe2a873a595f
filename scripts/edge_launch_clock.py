#!/usr/bin/env python3
"""Shader-clock stamps of the edge launches of one sigma call, in the order a replayed call runs them: the fused replace
launch (replace + coefficient table), the first think iteration, a steady one and the last one, at one workload's shape
with the engine's default noise stream.  Same instrumented library and stamp layout as scripts/shader_clock.py (thread 0 of
the first and of the last block; for the fused replace launch the first block is its table block).  Prints, per launch,
the wall time per launch of the replayed graph and the time from block entry to each stamp.  The think launches read the
generator state from the device words the replace launch publishes, as every launch of a replayed sigma call does (a launch
without a state pointer -- scripts/shader_clock.py -- does not show what that read costs).

    python scripts/edge_launch_clock.py [workload=c2_sdxl]
"""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lanpaint_amd import build as lpbuild            # noqa: E402

os.environ["LANPAINT_AMD_LIB"] = lpbuild.build(shader_clock=True, verbose=False)

import torch                                         # noqa: E402
import bench                                         # noqa: E402
from lanpaint_amd import _cabi                       # noqa: E402

STAMPS = ["kernel entry", "operand loads issued", "noise generated", "operands arrived", "stop verdict formed",
          "arithmetic done", "stores issued", "block sums written",      # (scripts/shader_clock.py; table block: 5 = table built)
          "generator started"]                                           # counter and seed in registers (one element per lane)


def descriptors(wl, dev):
    """replace (fused table), first, steady, last -- one descriptor each on shared buffers of the workload's shape"""
    R, F, S, P, E, K = (_cabi.LP_PH_REPLACE, _cabi.LP_PH_POST_FIRST, _cabi.LP_PH_POST_STEADY, _cabi.LP_PH_PRE_HALF,
                        _cabi.LP_PH_EMIT, _cabi.LP_PH_COEFFS)
    out, keep, state = [], [], None
    for name, ph in (("replace", R | E | K), ("first", F | P | E), ("steady", S | P | E), ("last", S | E)):
        d, k, n_el = bench.standalone_step(_cabi, wl, dev, ph, rng="torch")
        if ph & K:
            bufs, _m, coef, sig, ve, abt = k
            d.t_ve, d.t_abt, d.t_rsig, d.t_model = ve.data_ptr(), abt.data_ptr(), sig.data_ptr(), ve.data_ptr()
            d.t_ve_stride = d.t_abt_stride = d.t_rsig_stride = d.t_model_stride = 1
            d.coef_out = coef.data_ptr()
            state = torch.zeros(2, dtype=torch.int64, device=dev)
            d.rng_state_out, d.rng_state_val[0], d.rng_state_val[1] = state.data_ptr(), 0, 1234
            k = k + (state,)
        elif state is not None:
            d.rng_offset_ptr = state.data_ptr()
        out.append((name, d))
        keep.append(k)
    return out, keep, n_el


def main(wl):
    dev = torch.device("cuda", 0)
    lib = _cabi.load()
    launches, keep, n_el = descriptors(wl, dev)
    clk = torch.zeros((len(launches), 32), dtype=torch.float64, device=dev)
    for j, (_, d) in enumerate(launches):
        d.clk_out = clk[j].data_ptr()
    reps = 30

    def call():
        st = torch.cuda.current_stream(dev).cuda_stream
        for k in range(reps):
            for _, d in launches:
                d.rng_offset = 2 * k * d.rng_inc
                _cabi.check(lib.lp_step(ctypes.byref(d), st))

    call()
    torch.cuda.synchronize()
    g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.graph(g, stream=side):
        call()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        g.replay()
    torch.cuda.synchronize()
    us = (time.perf_counter() - t0) / (20 * reps) * 1e6
    print(f"{wl}: {us:.2f} us per sigma call of {len(launches)} dependent launches in a replayed graph (instrumented build)")
    h = clk.cpu().numpy()
    for j, (name, _) in enumerate(launches):
        print(f"\n{name}: last block entered {(h[j, 30] - h[j, 14]) * 10.0:.0f} ns after the first")
        for blk, o in (("first block" + (" (table block)" if name == "replace" else ""), h[j, 0:16]), ("last block", h[j, 16:32])):
            last = max(o[:len(STAMPS)])
            ns_per_tick = o[15] * 10.0 / last if last else 0.0
            stamps = ", ".join(f"{STAMPS[k]} {o[k] * ns_per_tick:.0f}" for k in range(1, len(STAMPS)) if o[k])
            print(f"  {blk}: span {o[15] * 10.0:.0f} ns; ns after entry: {stamps}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "c2_sdxl")
