"""Mask refine: grow or shrink a mask by a true Euclidean distance, then pull its edge onto the image underneath it.

Every node after the sampler takes the mask as given, and the mask is the one input nobody helps the user with: a painted mask
is a rough blob, a video mask between two keyframes is the SDF morph of two blobs and follows the subject's centroid, not its
outline.  Use this in front of the encode, a Detailer crop, the mask fill and the multiband blend, and behind the video mask
editor -- every frame is refined with that frame as its guide.

grow_mask(mask, grow) -> mask
        grow > 0: 1.0 where the nearest foreground pixel (v >= 0.5) is at most `grow` pixels away (Euclidean), else 0;
        grow < 0: 1.0 where the pixel is foreground and the nearest background pixel is more than |grow| away, else 0;
        grow == 0: the mask untouched, soft values kept.  Built on videomask.keyframe_edt's exact squared distances.
refine_mask(image, mask, radius=8, eps=1e-3, grow=0) -> mask [B, H, W]
        the grow first, then the colour guided filter (He et al.) of the mask with the image as the guide: inside every
        (2 radius + 1) window the mask is fitted as a linear function of the image's colour, and the fits are averaged.  Where
        the image has an edge within `radius` of the mask's, the mask's edge moves onto it; `eps` (in units of the [0, 1] image
        scale, squared) is how much colour variation counts as an edge -- larger values smooth more and snap less.  The rule
        works on 8-bit codes with exact integer sums and fp64 after them, so the result is the same bits on every run: an
        all-zero mask stays exactly 0, an all-one mask exactly 1, and nothing further than 2 radius pixels from the mask's soft
        region changes.  include/lanpaint_hip.h (lp_mask_refine) states the rule in full.

HIP tensors only, no CPU fallback.  The batch runs in chunks whose workspace stays under WS_CAP_BYTES; frames are independent,
so chunking cannot change a bit.
"""
from __future__ import annotations

import ctypes

import torch

from . import _cabi, videomask
from ._util import _as_f32c, raw_stream
from .detail import _mask3

MAX_SIDE = _cabi.LP_DETAIL_MAX_SIDE
MAX_RADIUS = _cabi.LP_REFINE_MAX_RADIUS
MAX_GROW = 256
EPS_RANGE = (1e-6, 1.0)
WS_CAP_BYTES = 1 << 30


def _hip(t, what):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"lanpaint_amd.refine runs on a HIP device only; no CPU fallback ({what} is not on one)")
    return t


def _int_in(v, lo, hi, what):
    if not isinstance(v, int) or isinstance(v, bool) or not lo <= v <= hi:
        raise ValueError(f"{what} must be an integer in {lo}..{hi}, got {v!r}")
    return v


def grow_mask(mask, grow):
    """`mask` [B, H, W], [1, H, W] or [H, W] grown (`grow` > 0) or shrunk (< 0) by |grow| pixels of Euclidean distance (module
    docstring); the shape is kept.  lp_vmask_edt's launches and torch comparisons on its int32 planes; no device -> host
    read."""
    _hip(mask, "mask")
    _int_in(grow, -MAX_GROW, MAX_GROW, "grow")
    if grow == 0:
        return mask
    m = _as_f32c(_mask3(mask))
    out = torch.empty_like(m)
    for s in range(0, m.shape[0], 65535):
        d2, _, _ = videomask.keyframe_edt(m[s:s + 65535])
        if grow > 0:
            near = d2[:, 0]
            on = (near >= 0) & (near <= grow * grow)
        else:
            far = d2[:, 1]
            on = (m[s:s + 65535] >= 0.5) & ((far > grow * grow) | (far == _cabi.LP_VMASK_D2_NONE))
        out[s:s + 65535] = on
    return out.reshape(mask.shape)


def refine_mask(image, mask, radius=8, eps=1e-3, grow=0):
    """The mask grown by `grow`, then guided-filtered with `image` as the guide (module docstring).  `image` [B, H, W, C] with
    C = 1 or C >= 3 (the first three channels are the guide), `mask` [B, H, W], [1, H, W] or [H, W]; fp32 [B, H, W] back.
    `radius` 0 returns the grown mask and launches no filter.  Two launches per chunk on the current stream and no
    device -> host read."""
    g = _hip(image, "image")
    _hip(mask, "mask")
    _int_in(radius, 0, MAX_RADIUS, "radius")
    _int_in(grow, -MAX_GROW, MAX_GROW, "grow")
    eps = float(eps)
    if not EPS_RANGE[0] <= eps <= EPS_RANGE[1]:
        raise ValueError(f"eps must lie in [{EPS_RANGE[0]}, {EPS_RANGE[1]}], got {eps!r}")
    if g.ndim != 4:
        raise ValueError(f"image must be [B, H, W, C], got {tuple(g.shape)}")
    B, H, W, C = g.shape
    if min(B, H, W) < 1 or max(H, W) > MAX_SIDE or C == 2 or not 1 <= C <= _cabi.LP_DETAIL_MAX_CHANNELS:
        raise ValueError(f"image {tuple(g.shape)}: sides 1..{MAX_SIDE}, channels 1 or 3..{_cabi.LP_DETAIL_MAX_CHANNELS}, batch >= 1")
    g = _as_f32c(g)
    dev = g.device
    m = _as_f32c(_mask3(mask).to(dev))
    if m.shape[0] not in (1, B) or tuple(m.shape[1:]) != (H, W):
        raise ValueError(f"mask shape {tuple(mask.shape)} does not match image {tuple(g.shape)}")
    m = grow_mask(m, grow)
    if radius == 0:
        return m.expand(B, H, W).clone()
    lib = _cabi.load()
    chunk = min(B, 65535, max(1, WS_CAP_BYTES // _cabi.refine_ws_bytes(1, H, W, C, radius)))
    ws_bytes = lib.lp_refine_ws_bytes(chunk, H, W, C, radius)
    _cabi.check(min(ws_bytes, 0), "lp_refine_ws_bytes")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    stream = raw_stream(dev)
    with torch.cuda.device(dev):
        for s in range(0, B, chunk):
            n = min(chunk, B - s)
            mc = m if m.shape[0] == 1 else m[s:s + n]
            d = _cabi.LpRefineDesc(n, H, W, C, mc.shape[0], radius, eps, g[s:s + n].data_ptr(), mc.data_ptr(),
                                   out[s:s + n].data_ptr(), ws.data_ptr(), ws_bytes)
            _cabi.check(lib.lp_mask_refine(ctypes.byref(d), stream), "lp_mask_refine")
    return out
