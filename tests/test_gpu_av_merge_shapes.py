"""lp_audio_merge on the MI355X against live references, at the sizes the recorded fixtures do not reach: the plan kernel with
several segments per thread (mask_len > 1024, per-sample masks at audio length), down-sampled long masks, windows wider than
the signal, the lane and block edges of the merge launch, operand strides with more than one batch, and one signal past
2^24 samples.  The reference is tests/audio_ref.py: torch's own index on the device in question, 0/1 masks counted in int64
(bit for bit), soft masks summed window by window in float64 (within one fp32 ulp plus the derived bound of the kernel's
prefix difference).  Reads no fixture file.  Every comparison covers every sample; each case prints one AV_MERGE line."""
import functools
import math

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, audio
from oracle import lanpaint_oracle as orc
from tests import audio_ref as ar
from tests.audio_ref import _reference_sequence
from tests.compare import ulps
from tests.device import DEV, _lib

pytestmark = pytest.mark.gpu

PLAN_THREADS = 1024                      # kPlanThreads of csrc/audio_kernel.hip: thread t owns ceil(fm / 1024) segments


# ---------------------------------------------------------------- helpers
@functools.lru_cache(maxsize=None)
def _zeros_ones(n):
    return torch.zeros(1, 1, n, device=DEV), torch.ones(1, 1, n, device=DEV)


def weights(am, n, cf):
    """w' as the kernel computes it (the merge of zeros into ones) for a mask on either device: crossfade cf seconds at a
    rate of 1 is cf samples."""
    z, o = _zeros_ones(n) if n <= 1 << 20 else (torch.zeros(1, 1, n, device=DEV), torch.ones(1, 1, n, device=DEV))
    return audio.merge_audio_with_mask(z, o, am, float(cf), 1, 1)[0, 0].cpu().numpy()


def weights_by_rule(am, n, cf, rule):
    """The same through audio._launch with a hand-made plan: any index rule, whatever host this runs on."""
    z, o = _zeros_ones(n)
    plan = audio.MergePlan(n=n, mask_len=int(am.shape[0]), batch=1, channels=1, cf=cf, nn_rule=rule, orig_strides=(0, 0),
                           inp_strides=(0, 0))
    return audio._launch(plan, am.to(DEV).contiguous(), z, o)[0, 0].cpu().numpy()


@functools.lru_cache(maxsize=64)
def src_live(fm, n, where):
    src = ar.src_index_live(fm, n, DEV if where == "device" else "cpu")
    src.setflags(write=False)
    return src


@functools.lru_cache(maxsize=64)
def src_generic(fm, n):
    src = np.arange(n, dtype=np.int64) if fm == n else orc.nearest_exact_src_index(n, fm, "generic")
    src.setflags(write=False)
    return src


def soft_mask(fm, seed, run=1):
    """rand with 30 % of the values times 1e-6; the scaled values come in runs of `run` entries (1: independent)."""
    rng = np.random.default_rng(seed)
    am = rng.random(fm, dtype=np.float32)
    quiet = (rng.random(-(-fm // run)) < 0.3).repeat(run)[:fm]
    am[quiet] *= np.float32(1e-6)
    return am


def report(tag, sizes, w, ref, bound):
    err = np.abs(w.astype(np.float64) - ref.astype(np.float64))
    u = ulps(w, ref)
    print(f"AV_MERGE {tag} {sizes} max_ulp={u.max():.1f} max_abs={err.max():.3g} bound={bound:.3g}")
    return err, u


def check_soft(tag, sizes, w, am, src, cf):
    """|w - w_ref| <= ulp32(w_ref) + weight_bound at every sample; returns the largest ulp distance."""
    ref = ar.weights_ref(am, src, cf)
    assert ref is not None, "no soft reference at this n * cf: shorten cf"
    bound = ar.weight_bound(am, src, cf)
    err, u = report(tag, sizes, w, ref, bound)
    assert np.all(err <= ar.ulp32(ref) + bound)
    return float(u.max())


def check_hard(tag, sizes, w, am, src, cf):
    ref = ar.weights_ref(am, src, cf)
    report(tag, sizes, w, ref, 0.0)
    assert np.array_equal(w, ref)


# ---------------------------------------------------------------- a. plan-kernel edges, hard masks, bit for bit
def _hard_masks(fm):
    rng = np.random.default_rng(fm)
    chunk = -(-fm // PLAN_THREADS)
    masks = [(rng.random(fm) < 0.5).astype(np.float32), (rng.random(fm) < 0.02).astype(np.float32),
             np.ones(fm, np.float32), np.zeros(fm, np.float32)]
    for at in sorted({0, fm - 1, chunk, chunk - 1}):          # a single 1: both ends and each side of a chunk boundary
        if 0 <= at < fm:
            m = np.zeros(fm, np.float32)
            m[at] = 1.0
            masks.append(m)
    return masks


@pytest.mark.parametrize("fm", [1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 3000, 5000])
def test_plan_kernel_edges_hard_masks(fm):
    """One, two, three and five segments per plan thread, a ragged last chunk, masks up-sampled, per sample and down-sampled
    (empty segments): every w' equals the int64 count, under the device's rule, the host's rule and the uncontracted one."""
    sizes = sorted({n for n in (fm, fm + 1, 2 * fm + 3, 7 * fm, fm - 1, fm // 2 + 1, 37) if n >= 1})
    masks = _hard_masks(fm)
    compared = wrong = 0
    for n in sizes:
        index = {"device": src_live(fm, n, "device"), "host": src_live(fm, n, "host"), "generic": src_generic(fm, n)}
        for src in index.values():
            assert src.shape == (n,) and src.min() >= 0 and src.max() <= fm - 1 and np.all(np.diff(src) >= 0)
        for cf in (0, 1, 2, 3, 44, 45):
            for k, am in enumerate(masks):
                t = torch.from_numpy(am)
                got = {"device": weights(t.to(DEV), n, cf), "host": weights(t, n, cf),
                       "generic": weights_by_rule(t, n, cf, _cabi.LP_NN_ATEN_CPU_GENERIC)}
                for path, w in got.items():
                    ref = ar.weights_ref(am, index[path], cf)
                    compared += 1
                    if not np.array_equal(w, ref):
                        wrong += 1
                        print(f"AV_MERGE plan_edges MISMATCH fm={fm} n={n} cf={cf} mask={k} {path} "
                              f"samples={int((w != ref).sum())} first={int(np.argmax(w != ref))}")
    print(f"AV_MERGE plan_edges fm={fm} chunk={-(-fm // PLAN_THREADS)} n={sizes} cf=(0,1,2,3,44,45) masks={len(masks)} "
          f"compared={compared} mismatched={wrong} max_ulp={'0.0' if not wrong else '>0'} max_abs=- bound=0")
    assert wrong == 0


# ---------------------------------------------------------------- b. per-sample masks at audio length
AUDIO_SIZES = [(48000, 48000), (480000, 480000), (250000, 480000), (480000, 250001)]


def _quiet_run(fm, n, cf):
    """Mask entries per quiet run, so that a run spans two windows of cf samples and some windows hold small values only."""
    return max(1, math.ceil(2 * cf * fm / n))


@pytest.mark.parametrize("cf", [960, 961])
@pytest.mark.parametrize("fm,n", AUDIO_SIZES)
def test_audio_length_hard_masks(fm, n, cf):
    """47 and 469 segments per plan thread (chunk = ceil(fm / 1024)), carried prefixes and the last chunk's ragged tail."""
    rng = np.random.default_rng(fm + n + cf)
    dense = (rng.random(fm) < 0.5).astype(np.float32)
    spans = (rng.random(-(-fm // 700)) < 0.4).repeat(700)[:fm].astype(np.float32)          # stretches longer than a chunk
    for name, am in (("dense", dense), ("spans", spans)):
        w = weights(torch.from_numpy(am).to(DEV), n, cf)
        check_hard(f"audio_hard_{name}", f"fm={fm} n={n} cf={cf}", w, am, src_live(fm, n, "device"), cf)


@pytest.mark.parametrize("cf", [960, 961])
@pytest.mark.parametrize("fm,n", AUDIO_SIZES)
def test_audio_length_soft_masks(fm, n, cf):
    """rand with 30 % of the values times 1e-6, within one fp32 ulp plus weight_bound of the direct float64 window sums.
    Values scaled independently never fill a whole window of 960 samples, so every w' would be near 0.35 and the prefix
    rounding invisible; here they come in runs two windows long, as a quiet stretch of a real mask does."""
    assert ar.has_soft_reference(n, cf)
    am = soft_mask(fm, fm + n + cf, _quiet_run(fm, n, cf))
    w = weights(torch.from_numpy(am).to(DEV), n, cf)
    check_soft("audio_soft", f"fm={fm} n={n} cf={cf}", w, am, src_live(fm, n, "device"), cf)


@pytest.mark.parametrize("fm,n,cf,run", [(250, 480000, 960, 1), (2047, 14329, 3, 1), (480000, 480000, 960, 2000)])
def test_long_soft_masks_are_not_within_two_ulps(fm, n, cf, run):
    """Why the soft criterion is one ulp plus a bound and not the 2 ulps of the short fixtures: where a whole window lies in
    a quiet stretch, w' is small and the rounding of the fp64 prefixes (of the size of the whole signal's sum) shows in its
    last fp32 places.  Harmless in absolute terms -- the same data is within ulp32 + weight_bound everywhere."""
    am = soft_mask(fm, 1, run)
    w = weights(torch.from_numpy(am).to(DEV), n, cf)
    worst = check_soft("audio_soft_two_ulps", f"fm={fm} n={n} cf={cf}", w, am, src_live(fm, n, "device"), cf)
    assert worst > 2


# ---------------------------------------------------------------- c. window against signal
@pytest.mark.parametrize("n", [1, 2, 3, 5, 300])
def test_window_against_signal(n):
    """cf around and far beyond n: both replicate clamps active in one window."""
    for cf in (n - 1, n, n + 1, 2 * n + 1, 48000):
        for fm in sorted({1, 6, n}):
            rng = np.random.default_rng(1000 * n + 7 * fm + cf)
            hard = (rng.random(fm) < 0.5).astype(np.float32)
            soft = soft_mask(fm, 1000 * n + fm)
            for where in ("device", "host"):
                src = src_live(fm, n, where)
                put = (lambda a: torch.from_numpy(a).to(DEV)) if where == "device" else torch.from_numpy
                sizes = f"fm={fm} n={n} cf={cf} {where}"
                check_hard("window_hard", sizes, weights(put(hard), n, cf), hard, src, cf)
                if cf > 1:
                    check_soft("window_soft", sizes, weights(put(soft), n, cf), soft, src, cf)
                else:
                    assert np.array_equal(weights(put(soft), n, cf), soft[src])


# ---------------------------------------------------------------- d. lane and block edges of the merge launch
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1020, 1023, 1024, 1025, 1027, 4099])
def test_lane_and_block_edges(n):
    """4 samples per lane, 256 lanes per block: the last lane's tail and the last block, once on aligned contiguous rows
    (float4 when n % 4 == 0) and once as a view one sample into longer rows (scalar)."""
    cf = 9
    g = torch.Generator(device="cpu").manual_seed(n)
    base_o, base_p = torch.randn(2, 2, n + 8, generator=g).to(DEV), torch.randn(2, 2, n + 8, generator=g).to(DEV)
    am = soft_mask(7, n)
    view_o, view_p = base_o[..., 1:n + 1], base_p[..., 1:n + 1]
    assert view_o.data_ptr() % 16 != 0 and view_o.stride(1) == n + 8
    o, p = view_o.contiguous(), view_p.contiguous()
    assert o.data_ptr() % 16 == 0 and p.data_ptr() % 16 == 0
    mask = torch.from_numpy(am).to(DEV)
    a = audio.merge_audio_with_mask(o, p, mask, float(cf), 1, 1).cpu().numpy()
    b = audio.merge_audio_with_mask(view_o, view_p, mask, float(cf), 1, 1).cpu().numpy()
    w = weights(mask, n, cf)
    check_soft("lane_edges", f"fm=7 n={n} cf={cf}", w, am, src_live(7, n, "device"), cf)
    assert a.shape == (2, 2, n)
    assert np.array_equal(a, b)
    assert np.array_equal(a, ar.merge_ref(o.cpu().numpy(), p.cpu().numpy(), w))


# ---------------------------------------------------------------- e. strides
def _stride_cases():
    n, L = 1000, 1012
    g = torch.Generator(device="cpu").manual_seed(77)

    def rand(*shape):
        return torch.randn(*shape, generator=g).to(DEV)
    yield "six_channels_cut_three_batches", rand(3, 6, L)[..., :n], rand(3, 2, n)
    yield "batch_broadcast_orig", rand(1, 2, n), rand(3, 2, n)
    yield "batch_broadcast_inp", rand(3, 2, n), rand(1, 2, n)
    yield "mono_orig", rand(3, 1, n), rand(3, 2, n)
    yield "mono_inp", rand(3, 2, n), rand(3, 1, n)
    yield "mono_and_batch_broadcast_orig", rand(1, 1, n), rand(3, 2, n)
    yield "mono_and_batch_broadcast_inp", rand(3, 2, n), rand(1, 1, n)
    yield "both_broadcast_crosswise", rand(1, 2, n), rand(3, 1, n)
    o = rand(3, 2, L)[..., 1:n + 1]                   # row stride 1012 (a multiple of 4), base 4 bytes past a 16 B boundary
    assert o.stride(1) % 4 == 0 and o.stride(0) % 4 == 0 and o.data_ptr() % 16 != 0
    yield "stride_of_4_misaligned_base", o, rand(3, 2, n)
    o = rand(3, 2, L + 1)[..., :n]                    # aligned base, odd row stride
    assert o.stride(1) % 4 != 0 and o.data_ptr() % 16 == 0
    yield "aligned_base_odd_stride", o, rand(3, 2, n)
    p = rand(3, 2, L)[..., 1:n + 1]
    yield "misaligned_inp_only", rand(3, 2, n), p


@pytest.mark.parametrize("cf", [0, 25])
def test_strides(cf):
    """Truncated, channel-cut, broadcast and misaligned operands with more than one batch: the same bits as the call on
    contiguous copies, and as the fp32 lerp of the reference's channel / batch rule on the kernel's own w'."""
    n = 1000
    am = soft_mask(13, 5)
    mask = torch.from_numpy(am).to(DEV)
    w = weights(mask, n, cf)
    src = src_live(13, n, "device")
    if cf > 1:
        check_soft("strides_w", f"fm=13 n={n} cf={cf}", w, am, src, cf)
    else:
        assert np.array_equal(w, am[src])
    for name, o, p in _stride_cases():
        got = audio.merge_audio_with_mask(o, p, mask, float(cf), 1, 1).cpu().numpy()
        flat = audio.merge_audio_with_mask(o.contiguous(), p.contiguous(), mask, float(cf), 1, 1).cpu().numpy()
        want = ar.merge_ref(o.cpu().numpy(), p.cpu().numpy(), w)
        assert got.shape == want.shape == (3, 2, n), name
        print(f"AV_MERGE strides {name} cf={cf} orig={tuple(o.shape)}/{tuple(o.stride())} inp={tuple(p.shape)}/{tuple(p.stride())} "
              f"max_ulp={ulps(got, want).max():.1f} max_abs={np.abs(got - want).max():.3g} bound=0")
        assert np.array_equal(got, flat), name
        assert np.array_equal(got, want), name


# ---------------------------------------------------------------- f. one case past 2^24
@pytest.mark.parametrize("fm", [7, 2049])
def test_past_two_to_the_24(fm):
    """n = 2^24 + 12, the smallest size at which float(i) is inexact for some sample: the segment starts come from the
    fix-up walk over the index as the device's own interpolate rounds it."""
    n = 2 ** 24 + 12
    rng = np.random.default_rng(fm)
    am = (rng.random(fm) < 0.5).astype(np.float32)
    am[-1] = 1.0 - am[-2]                                   # a transition in the last samples, where float(i) rounds
    mask = torch.from_numpy(am).to(DEV)
    src = ar.src_index_live(fm, n, DEV)
    assert np.all(np.diff(src) >= 0) and src[0] == 0 and src[-1] == fm - 1
    w0 = weights(mask, n, 0)
    report("past_2^24", f"fm={fm} n={n} cf=0", w0, am[src], 0.0)
    assert np.array_equal(w0, am[src])
    del w0
    check_hard("past_2^24", f"fm={fm} n={n} cf=960", weights(mask, n, 960), am, src, 960)


# ---------------------------------------------------------------- g. the live torch sequence
@pytest.mark.parametrize("kind", ["hard", "soft"])
def test_long_mask_against_the_torch_sequence(kind):
    fm, n, sr, crossfade = 2049, 96000, 48000, 0.02
    assert audio.crossfade_samples(crossfade, sr) == 960
    g = torch.Generator(device="cpu").manual_seed(11)
    orig, inp = (0.3 * torch.randn(2, 2, n, generator=g)).to(DEV), (0.3 * torch.randn(2, 2, n, generator=g)).to(DEV)
    am = soft_mask(fm, 3) if kind == "soft" else (np.random.default_rng(3).random(fm) < 0.5).astype(np.float32)
    mask = torch.from_numpy(am).to(DEV)
    want, want_w = _reference_sequence(orig, inp, mask, crossfade, sr)
    got = audio.merge_audio_with_mask(orig, inp, mask, crossfade, sr, sr)
    w = audio.merge_audio_with_mask(torch.zeros(1, 1, n, device=DEV), torch.ones(1, 1, n, device=DEV), mask, crossfade, sr,
                                    sr)[0, 0].cpu().numpy()
    report(f"torch_sequence_{kind}", f"fm={fm} n={n} cf=960", w, want_w.cpu().numpy(), 3e-5)
    np.testing.assert_allclose(w, want_w.cpu().numpy(), rtol=0, atol=3e-5)
    np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=0, atol=1e-4)
    assert np.array_equal(got.cpu().numpy(), ar.merge_ref(orig.cpu().numpy(), inp.cpu().numpy(), w))
