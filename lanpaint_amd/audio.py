"""Audio merge of the AV decode on the GPU.

Restates the reference's `merge_audio_with_mask` (src/LanPaint/nodes.py:1091-1136, run by LanPaint_AVDecode): the inpainted
waveform replaces the original inside the audio mask, with a box crossfade of `crossfade` seconds at the mask's edges.

  1. the inpainted audio is brought to the original's rate (torchaudio.functional.resample, as the reference does) and both
     waveforms are cut to the shorter length;
  2. the mask ([F], [F, 1] or SetLatentNoiseMask's [1, 1, F, 1]) is normalised to [F] on the host -- a plan of sizes, the
     crossfade width in samples, the index rule and per-operand strides (`plan_merge`);
  3. one lp_audio_merge job (csrc/audio_kernel.hip) up-samples the mask nearest-exact, crossfades it and blends every channel.

The channel rule is the reference's: a mono side is broadcast, otherwise the original's first channels are kept.  Broadcasts
are zero strides: neither waveform is copied.  HIP tensors only, no CPU fallback; the result stays on the device.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import torch

from . import _cabi, interp_rule
from ._hostcall import launch, node_device

try:
    import torchaudio
except ImportError:                    # optional: only needed when the two sample rates differ
    torchaudio = None


def normalize_mask(mask):
    """The audio mask as a 1-D float tensor on its own device: [F] as given, [F, 1] -> [F], and SetLatentNoiseMask's
    [1, 1, F, 1] -> [F] (the reference documents that form but its interpolate call rejects it; accepted here)."""
    m = torch.as_tensor(mask).float()
    if m.ndim == 4 and m.shape[0] == 1 and m.shape[1] == 1 and m.shape[3] == 1:
        m = m[0, 0, :, 0]
    elif m.ndim == 2 and m.shape[1] == 1:
        m = m[:, 0]
    if m.ndim != 1:
        raise ValueError(f"the audio mask must be [F], [F, 1] or [1, 1, F, 1], got {tuple(mask.shape)}")
    if m.shape[0] < 1:
        raise ValueError("the audio mask is empty")
    return m


def crossfade_samples(crossfade, orig_sr):
    """Width of the box crossfade in samples, computed as the reference does; 0 = none (a width of 1 is the identity)."""
    if crossfade > 0 and orig_sr > 0:
        return max(1, int(round(crossfade * orig_sr)))
    return 0


@dataclass
class MergePlan:
    n: int
    mask_len: int
    batch: int
    channels: int
    cf: int
    nn_rule: int
    orig_strides: tuple          # (batch, channel) element strides, 0 = broadcast
    inp_strides: tuple


def _broadcast(a, b, what):
    if a == b or b == 1:
        return a
    if a == 1:
        return b
    raise RuntimeError(f"the original and the inpainted audio cannot be merged: {what} {a} vs {b}")


def plan_merge(orig, inpainted, am, cf, nn_rule):
    """Output shape and operand strides of `orig * (1 - w) + inpainted * w` after the reference's channel matching, for
    [B, C, n] waveforms of equal length whose samples are contiguous; `am` the normalised [F] mask."""
    n = int(orig.shape[-1])
    if orig.ndim != 3 or inpainted.ndim != 3 or int(inpainted.shape[-1]) != n:
        raise ValueError(f"expected [B, C, L] waveforms of one length, got {tuple(orig.shape)} and {tuple(inpainted.shape)}")
    if n < 1:
        raise ValueError("the audio is empty")
    co, ci = int(orig.shape[1]), int(inpainted.shape[1])
    if co != ci and co != 1 and ci != 1:
        co = min(co, ci)                         # surround original vs fewer inpainted channels: orig[:, :Ci]
    channels = _broadcast(co, ci, "channels")
    batch = _broadcast(int(orig.shape[0]), int(inpainted.shape[0]), "batch")

    def strides(t, c):
        return (0 if t.shape[0] == 1 else int(t.stride(0)), 0 if c == 1 else int(t.stride(1)))
    return MergePlan(n=n, mask_len=int(am.shape[0]), batch=batch, channels=channels, cf=int(cf), nn_rule=int(nn_rule),
                     orig_strides=strides(orig, co), inp_strides=strides(inpainted, ci))


def _launch(plan, m, o, p):
    dev = o.device
    out = torch.empty((plan.batch, plan.channels, plan.n), dtype=torch.float32, device=dev)
    ws = torch.empty(_cabi.lp_audio_ws_bytes(plan.mask_len), dtype=torch.uint8, device=dev) if plan.cf > 1 else None
    d = _cabi.LpAudioDesc()
    d.n, d.mask_len, d.batch, d.channels, d.cf, d.nn_rule = (plan.n, plan.mask_len, plan.batch, plan.channels, plan.cf,
                                                             plan.nn_rule)
    d.orig_sb, d.orig_sc = plan.orig_strides
    d.inp_sb, d.inp_sc = plan.inp_strides
    d.mask, d.orig, d.inpainted, d.out = m.data_ptr(), o.data_ptr(), p.data_ptr(), out.data_ptr()
    d.workspace = ws.data_ptr() if ws is not None else None
    launch("lp_audio_merge", dev, ctypes.byref(d))
    return out


def merge_audio_with_mask(orig, inpainted, mask, crossfade, orig_sr, result_sr):
    """nodes.py:1091-1136: `orig` / `inpainted` are [B, C, L] waveforms at `orig_sr` / `result_sr`, `mask` the per-frame
    audio mask (1 = take the inpainted audio).  Returns the merged [B', C', n] fp32 waveform on the HIP device."""
    if result_sr != orig_sr:
        if torchaudio is None:
            raise RuntimeError("torchaudio is required to resample the inpainted audio")
        inpainted = torchaudio.functional.resample(inpainted, result_sr, orig_sr)
    n = min(int(inpainted.shape[-1]), int(orig.shape[-1]))
    orig, inpainted = orig[..., :n], inpainted[..., :n]
    am = normalize_mask(mask)
    cf = crossfade_samples(crossfade, orig_sr)
    # the reference up-samples the mask with a 1-D F.interpolate on the MASK's device: the kernel follows that kernel's rule
    rule = interp_rule.rule_for(am, am.reshape(1, 1, -1), (n,)) if am.shape[0] != n else _cabi.LP_NN_ATEN_SCALAR
    plan_merge(orig, inpainted, am, cf, rule)            # shape errors surface before anything touches the device
    dev = node_device(orig)

    def on_device(t):
        t = t.to(device=dev, dtype=torch.float32)
        return t if t.stride(-1) == 1 else t.contiguous()
    o, p, m = on_device(orig), on_device(inpainted), on_device(am).contiguous()
    return _launch(plan_merge(o, p, m, cf, rule), m, o, p)    # the strides of the device copies
