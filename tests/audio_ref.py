"""A reference for lp_audio_merge that shares nothing with the kernel (no GPU needed).

Written from the formula of include/lanpaint_hip.h (lp_audio_desc), not from csrc/audio_kernel.hip: the source index is asked
of torch itself on the device in question, and the crossfade's window sum never goes through a whole-signal fp64 prefix --
the kernel's own idea, whose cancellation a restatement built the same way (weights_f64 below) shares.

  src_index_live   the nearest-exact source index as torch computes it on a device
  weights_ref      w' = float32(S * float64(float32(1) / float32(cf))), S counted in int64 (0/1 masks, exact) or summed
                   window by window in float64 (soft masks, torch's replicate pad + conv1d)
  weight_bound     how far a prefix-difference evaluation of S may be from that for a soft mask
  merge_ref        the reference's channel / batch rule and the fp32 lerp

Below them, what the host test and the kernel tests of the audio merge share: the fixtures' loader, the prefix-sum restatement
(weights_f64, lerp_f32, restated_merge, host_rule) and the reference sequence of the shape tests.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from lanpaint_amd import _cabi, audio, interp_rule
from oracle import lanpaint_oracle as orc

SOFT_LIMIT = 5e8               # n * cf above which no direct float64 window sum is taken (time and memory of the host conv1d)
_CONV_OUT = 1 << 15            # outputs per conv1d call: bounds the im2col buffer of torch's float64 convolution


def src_index_live(fm, n, device):
    """int64 [n] numpy: the source index of every sample as torch's nearest-exact kernel picks it on `device`.  An arange
    of fm < 2^24 values is exact in fp32, so interpolating it returns the index itself.  fm == n: the identity (the
    reference takes a per-sample mask as given)."""
    if fm == n:
        return np.arange(n, dtype=np.int64)
    assert fm < 2 ** 24
    ramp = torch.arange(fm, dtype=torch.float32, device=device)[None, None]
    return F.interpolate(ramp, size=(n,), mode="nearest-exact")[0, 0].to(torch.int64).cpu().numpy()


def is_hard(am):
    am = np.asarray(am)
    return bool(np.all((am == 0) | (am == 1)))


def ulp32(x):
    """The fp32 unit in the last place at |x|, as float64."""
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


def _window(n, cf):
    i = np.arange(n, dtype=np.int64)
    lo_raw = i - cf // 2
    hi_raw = lo_raw + cf
    return lo_raw, hi_raw, np.maximum(lo_raw, 0), np.minimum(hi_raw, n)


def has_soft_reference(n, cf):
    return cf <= 1 or n * cf <= SOFT_LIMIT


def weights_ref(am, src, cf):
    """float32 [n]: w' of the header for the mask `am` [fm] and the source index `src` [n].  Returns None for a soft mask
    with n * cf > SOFT_LIMIT: no direct window sum is taken at that size (the hard mask covers it)."""
    am = np.asarray(am, np.float32)
    src = np.asarray(src, np.int64)
    w = am[src]
    n = w.shape[0]
    if cf <= 1:
        return w
    tap = np.float64(np.float32(1) / np.float32(cf))
    if is_hard(am):                                # every term an integer: an int64 count is the exact window sum
        c = np.concatenate([[0], np.cumsum(w.astype(np.int64))])
        lo_raw, hi_raw, lo, hi = _window(n, cf)
        S = (lo - lo_raw) * int(w[0]) + (hi_raw - hi) * int(w[-1]) + (c[hi] - c[lo])
        return (S.astype(np.float64) * tap).astype(np.float32)
    if not has_soft_reference(n, cf):
        return None
    # soft values: torch's own replicate pad, then each window summed on its own in float64 (conv1d with a kernel of ones),
    # a slice of outputs at a time
    wp = F.pad(torch.from_numpy(w.astype(np.float64))[None, None], (cf // 2, cf - 1 - cf // 2), mode="replicate")
    ones = torch.ones(1, 1, cf, dtype=torch.float64)
    S = torch.empty(n, dtype=torch.float64)
    for a in range(0, n, _CONV_OUT):
        b = min(n, a + _CONV_OUT)
        S[a:b] = F.conv1d(wp[..., a:b + cf - 1], ones)[0, 0]
    return (S.numpy() * tap).astype(np.float32)


def weight_bound(am, src, cf):
    """The absolute distance a prefix-difference evaluation of S may add for a soft mask, beyond the final fp32 rounding:
    (fm + 4) * 2^-52 * sum_s |am[s]| * len(s) / cf -- fm rounded fp64 additions on a prefix no larger than the sum of
    |w| over the signal, each off by at most 2^-53 of it, in both prefixes of the difference.  0 for a 0/1 mask or no
    crossfade: those are exact."""
    am = np.asarray(am, np.float32)
    if cf <= 1 or is_hard(am):
        return 0.0
    total = float(np.abs(am[np.asarray(src, np.int64)].astype(np.float64)).sum())       # sum_s |am[s]| * len(s)
    return (am.shape[0] + 4) * 2.0 ** -52 * total / cf


def merge_ref(orig, inp, w):
    """The reference's blend on numpy arrays [B, C, n]: a mono side is expanded, otherwise the original's first channels
    are kept; batches broadcast; o * (1 - w) + p * w with each product and the sum rounded in fp32."""
    o, p = np.asarray(orig, np.float32), np.asarray(inp, np.float32)
    if o.shape[1] != p.shape[1] and o.shape[1] != 1 and p.shape[1] != 1:
        o = o[:, :p.shape[1]]
    return lerp_f32(o, p, np.asarray(w, np.float32)[None, None])


RULE_NAMES = {_cabi.LP_NN_ATEN_SCALAR: "scalar", _cabi.LP_NN_ATEN_CPU_GENERIC_FMA: "generic_fma",
              _cabi.LP_NN_ATEN_CPU_GENERIC: "generic"}


def fixture_id(path):
    return os.path.basename(path)[len("av_merge_"):-4]


def load_fixture(path):
    z = np.load(path)
    return {k: z[k] for k in z.files}


def weights_f64(am, n, cf, rule):
    """w' of include/lanpaint_hip.h (lp_audio_desc): the up-sampled mask, then float(S * double(1.0f / cf)) with S the
    replicate-clamped window sum, here from a plain float64 cumulative sum over the samples."""
    am = np.asarray(am, np.float32)
    w = am if am.shape[0] == n else am[orc.nearest_exact_src_index(n, am.shape[0], RULE_NAMES[rule])]
    w = w.astype(np.float64)
    if cf <= 1:
        return w.astype(np.float32)
    c = np.concatenate([[0.0], np.cumsum(w)])
    i = np.arange(n, dtype=np.int64)
    lo_raw = i - cf // 2
    hi_raw = lo_raw + cf
    lo, hi = np.maximum(lo_raw, 0), np.minimum(hi_raw, n)
    s = (lo - lo_raw) * w[0] + (hi_raw - hi) * w[-1] + (c[hi] - c[lo])
    return (s * np.float64(np.float32(1.0) / np.float32(cf))).astype(np.float32)


def lerp_f32(o, p, w):
    """o * (1 - w) + p * w in fp32, every operation rounded (what torch's separate ops do)."""
    w = np.asarray(w, np.float32)
    return (o.astype(np.float32) * (np.float32(1) - w) + p.astype(np.float32) * w).astype(np.float32)


def restated_merge(rec, rule):
    """The whole merge on equal-rate inputs, restated on numpy arrays with the reference's channel rule."""
    o, p = rec["orig"], rec["inpainted"]
    n = min(o.shape[-1], p.shape[-1])
    o, p = o[..., :n], p[..., :n]
    am = audio.normalize_mask(torch.from_numpy(rec["mask"])).numpy()
    w = weights_f64(am, n, audio.crossfade_samples(float(rec["crossfade"]), int(rec["orig_sr"])), rule)
    if o.shape[1] != p.shape[1] and o.shape[1] != 1 and p.shape[1] != 1:
        o = o[:, :p.shape[1]]
    return lerp_f32(o, p, w[None, None]), w


def host_rule(rec):
    """The index rule torch's CPU kernel takes for the fixtures' host masks (what the reference ran)."""
    am = audio.normalize_mask(torch.from_numpy(rec["mask"]))
    n = min(rec["orig"].shape[-1], rec["inpainted"].shape[-1])
    return interp_rule.rule_for(am, am.reshape(1, 1, -1), (n,))


def _reference_sequence(orig, inp, am, crossfade, sr):
    """The reference's merge_audio_with_mask as a torch sequence (equal rates), run wherever its tensors are."""
    n = orig.shape[-1]
    w = torch.nn.functional.interpolate(am[None, None], size=(n,), mode="nearest-exact")[0, 0]
    cf = max(1, int(round(crossfade * sr)))
    k = torch.ones(1, 1, cf, device=orig.device) / cf
    w = torch.nn.functional.conv1d(torch.nn.functional.pad(w[None, None], (cf // 2, cf - 1 - cf // 2), mode="replicate"), k)[0, 0]
    return orig * (1 - w[None, None]) + inp * w[None, None], w
