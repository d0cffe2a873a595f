"""The measuring kit of the feature benchmarks (scripts/bench_*.py): timers, series, launch counts, the command line.

A benchmark script holds its workloads, the torch-operator restatement of its rule, its expected-launch formulas and its
measure(); how a time is taken is stated here, once, and every script takes its times this way.

    wall(fn)         host clock, ms: a device synchronise, the clock, the call, a device synchronise, the clock.  It includes
                     the host's work in the call, every launch gap and the wait for the device to drain.
    events(fn, reps) device events, ms per call: an event recorded on the current stream, `reps` back-to-back calls, an event,
                     and the host waits for the second.  It includes what the stream does between the two records -- kernels
                     and the gaps between dependent launches -- but not host work that ends before the first kernel starts.
    series           an ordered list of (tag, fn): `warmup` untimed rounds, a synchronise, `iters` timed rounds; every round
                     walks the whole list, so the tags' samples interleave in time.
    spread           a run-to-run spread comes from two interleaved series of the SAME code under two tags (`x_a`, `x_b`) in one
                     list: the relative difference of their medians.  It is what a difference between two sides has to exceed
                     to mean anything.  A script reports min..max of the samples next to it.
    --job            runs one body only, warm-up plus iterations, and prints nothing: the body of a profiler run
                     (rocprofv3 --kernel-trace --stats -- python scripts/bench_X.py --job ...).

Importing this module puts the repository root and scripts/ on sys.path; torch is imported where it is first needed.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "scripts"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

median = statistics.median


# ---- timers ------------------------------------------------------------------------------------------------------------------
def synchronize():
    import torch
    torch.cuda.synchronize()


def events(fn, reps=1):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    e1.synchronize()
    del out
    return e0.elapsed_time(e1) / reps


def wall(fn, clock=time.perf_counter, sync=synchronize):
    sync()
    t0 = clock()
    out = fn()
    sync()
    del out
    return (clock() - t0) * 1e3


# ---- series ------------------------------------------------------------------------------------------------------------------
def series(order, iters, warmup, timer=events, sync=synchronize):
    """`order` is a list of (tag, fn), or (tag, fn, timer) where a list mixes clocks.  Every fn runs untimed, in order, for `warmup`
    rounds; then one synchronise; then `iters` rounds of timer(fn) in order.  Returns {tag: [ms per round]}."""
    for _ in range(warmup):
        for _, fn, *_ in order:
            fn()
    sync()
    rec = {tag: [] for tag, *_ in order}
    for _ in range(iters):
        for tag, fn, *own in order:
            rec[tag].append((own[0] if own else timer)(fn))
    return rec


def untimed(fn, rounds):
    """`rounds` calls and a synchronise: a warm-up that differs from the timed list, or the body of a profiler run."""
    series([("", fn)], 0, rounds)


def spread(a, b, digits=4):
    """Two series of the same code: the relative difference of their medians, over the median of all their samples."""
    return round(abs(median(a) - median(b)) / median(a + b), digits)


def summary(samples, digits=4):
    """(median, [min, max]) of a sample list, rounded for the JSON line."""
    return round(median(samples), digits), [round(min(samples), digits), round(max(samples), digits)]


# ---- counts ------------------------------------------------------------------------------------------------------------------
def count_launches(fn, *modules):
    """The entry names `fn` launches from `modules` (lanpaint_amd.propagate when none is named) and from the motion layer they
    share, in call order: every module binds `launch` by name, so each one's own name is wrapped."""
    from lanpaint_amd import _motion, propagate
    real = {m: m.launch for m in (*(modules or (propagate,)), _motion)}
    names = []
    for m, f in real.items():
        m.launch = lambda entry, *a, f=f: (names.append(entry), f(entry, *a))[1]
    try:
        fn()
    finally:
        for m, f in real.items():
            m.launch = f
    return names


def differing(a, b):
    """How many elements of two tensors (or of two tuples of tensors, pairwise) differ, a NaN equal to a NaN."""
    if isinstance(a, (tuple, list)):
        return sum(differing(x, y) for x, y in zip(a, b))
    return int(((a != b) & ~((a != a) & (b != b))).sum())


# ---- command line ------------------------------------------------------------------------------------------------------------
def parser(cases=None, jobs=None, iters=10, warmup=2):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=iters)
    ap.add_argument("--warmup", type=int, default=warmup)
    if cases:
        ap.add_argument("--case", choices=tuple(cases), help="this workload only")
    if jobs:
        ap.add_argument("--job", choices=tuple(jobs), help="run this body only and print nothing (a profiler run's body)")
    return ap


def device(hint=""):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit(f"{os.path.basename(sys.argv[0])} needs a HIP device{hint}")
    return torch.device("cuda", 0)


def emit(metric, a, cases=None, **extra):
    import torch
    line = {"metric": metric, "unit": "ms", "device": torch.cuda.get_device_name(0)}
    if a is not None:                                                   # a script with per-side iteration counts states them there
        line.update(iters=a.iters, warmup=a.warmup)
    if cases is not None:
        line["cases"] = cases
    print(json.dumps({**line, **extra}, separators=(",", ":")))
