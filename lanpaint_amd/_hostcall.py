"""What the image-space modules (video mask, audio merge, blend, Detailer, colour match, fill, multiband, refine, stabilize) and
their nodes share between a node and a C entry point: the device rule, argument checks, the launch, workspaces and chunking.
Plain functions; nothing of the engine's path is here (that is _util.py's).  HIP tensors only, no CPU fallback.  The motion
modules (the propagates, the temporal fills and smooths, shot detection) use these too; what only they share -- the block
matcher's checks, the luma pyramids, the batched field walk -- is the layer next to this one, _motion.py."""
from __future__ import annotations

import math

import torch

from . import _cabi
from ._util import _as_f32c, raw_stream

MAX_BATCH = 65535                     # the most images one launch takes: a grid's y / z limit


def require_hip(t, what, module):
    """`t` when it is a tensor on a HIP device; `module` is the caller's __name__, `what` its argument."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"{module} runs on a HIP device only; no CPU fallback ({what} is not on one)")
    return t


def tensor_is(t, dtype, shape, what, module):
    """`t` when it is a contiguous tensor of `dtype` and exactly `shape` on a HIP device; a None in `shape` leaves that
    dimension free.  `what` names the argument, `module` is the caller's __name__."""
    require_hip(t, what, module)
    fits = t.shape == shape                                          # the usual case in one comparison: this runs before every launch
    if not fits and t.ndim == len(shape):
        fits = all(n is None or n == s for n, s in zip(shape, t.shape))
    if not fits or t.dtype != dtype or not t.is_contiguous():
        want = ", ".join("n" if n is None else str(n) for n in shape)
        raise ValueError(f"{what} must be a contiguous {dtype} [{want}], got {t.dtype} {list(t.shape)}")
    return t


def node_device(t, device=None):
    """The device a node works on: `device` when it names a HIP device, else t's own when it is on one, else the current one."""
    if device is not None and torch.device(device).type == "cuda":
        return torch.device(device)
    if t.is_cuda:
        return t.device
    if not torch.cuda.is_available():
        raise RuntimeError("the LanPaint nodes run on a HIP device only; no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def node_mask(mask, dev):
    """A node's MASK input, [H, W] or [B, H, W], as [B, H, W] on `dev`."""
    return (mask.unsqueeze(0) if mask.ndim == 2 else mask).to(dev)


def int_in(v, lo, hi, what):
    if not isinstance(v, int) or isinstance(v, bool) or not lo <= v <= hi:
        raise ValueError(f"{what} must be an integer in {lo}..{hi}, got {v!r}")
    return v


def float_in(v, lo, hi, what):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or math.isnan(v) or not lo <= v <= hi:
        raise ValueError(f"{what} must be a number in {lo}..{hi}, got {v!r}")
    return float(v)


def mask3(mask):
    if mask.ndim == 2:
        return mask.unsqueeze(0)
    if mask.ndim != 3:
        raise ValueError(f"mask must be [B, H, W], [1, H, W] or [H, W], got {tuple(mask.shape)}")
    return mask


def image4(t, what, max_batch=None):
    """`t` when it is [B, H, W, C] within the kernels' side and channel limits and, with `max_batch`, that batch limit."""
    if t.ndim != 4:
        raise ValueError(f"{what} must be [B, H, W, C], got {tuple(t.shape)}")
    b, h, w, c = t.shape
    side, chan = _cabi.LP_DETAIL_MAX_SIDE, _cabi.LP_DETAIL_MAX_CHANNELS
    if min(b, h, w, c) < 1 or max(h, w) > side or c > chan or (max_batch is not None and b > max_batch):
        raise ValueError(f"{what} {tuple(t.shape)}: sides 1..{side}, channels 1..{chan}, batch "
                         + (f"1..{max_batch}" if max_batch is not None else ">= 1"))
    return t


def mask_for(mask, B, H, W, dev):
    """`mask` ([B, H, W], [1, H, W] or [H, W]) as contiguous fp32 on `dev`: one plane for all B images of H x W, or one each."""
    m = _as_f32c(mask3(mask).to(dev))
    if m.shape[0] not in (1, B) or tuple(m.shape[1:]) != (H, W):
        raise ValueError(f"mask shape {tuple(mask.shape)} does not match {B} images of {H}x{W}")
    return m


def launch(entry, dev, *args):
    """The C entry `entry` called with `args` and torch's current stream on `dev`; a negative status raises."""
    with torch.cuda.device(dev):
        _cabi.check(getattr(_cabi.load(), entry)(*args, raw_stream(dev)), entry)


def workspace(ws_bytes, dev, what="workspace size"):
    """`ws_bytes` of device memory, as a *_ws_bytes entry counted them; a negative count is its status and raises."""
    _cabi.check(min(ws_bytes, 0), what)
    return torch.empty(ws_bytes, dtype=torch.uint8, device=dev)


def chunks(n, per_item_bytes, cap_bytes):
    """(start, count) over `n` items, as many at a time as stay under `cap_bytes` and MAX_BATCH, at least one."""
    step = min(MAX_BATCH, max(1, cap_bytes // per_item_bytes))
    for s in range(0, n, step):
        yield s, min(step, n - s)
