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

HIP tensors only, no CPU fallback.  The batch runs in chunks that keep the filter's workspace, and the grow's distance buffers
(videomask.edt_chunks), under WS_CAP_BYTES; frames are independent, so chunking cannot change a bit.
"""
from __future__ import annotations

import ctypes

import torch

from . import _cabi, videomask
from ._hostcall import chunks, image4, int_in, launch, mask3, mask_for, require_hip, workspace
from ._util import _as_f32c

MAX_SIDE = _cabi.LP_DETAIL_MAX_SIDE
MAX_RADIUS = _cabi.LP_REFINE_MAX_RADIUS
MAX_GROW = 256
EPS_RANGE = (1e-6, 1.0)
WS_CAP_BYTES = 1 << 30


def grow_mask(mask, grow):
    """`mask` [B, H, W], [1, H, W] or [H, W] grown (`grow` > 0) or shrunk (< 0) by |grow| pixels of Euclidean distance (module
    docstring); the shape is kept.  lp_vmask_edt's launches and torch comparisons on its int32 planes; no device -> host
    read."""
    require_hip(mask, "mask", __name__)
    int_in(grow, -MAX_GROW, MAX_GROW, "grow")
    if grow == 0:
        return mask
    m = _as_f32c(mask3(mask))
    out = torch.empty_like(m)
    for s, n, d2 in videomask.edt_chunks(m, WS_CAP_BYTES):
        if grow > 0:
            near = d2[:, 0]
            on = (near >= 0) & (near <= grow * grow)
        else:
            far = d2[:, 1]
            on = (m[s:s + n] >= 0.5) & ((far > grow * grow) | (far == _cabi.LP_VMASK_D2_NONE))
        out[s:s + n] = on
    return out.reshape(mask.shape)


def refine_mask(image, mask, radius=8, eps=1e-3, grow=0):
    """The mask grown by `grow`, then guided-filtered with `image` as the guide (module docstring).  `image` [B, H, W, C] with
    C = 1 or C >= 3 (the first three channels are the guide), `mask` [B, H, W], [1, H, W] or [H, W]; fp32 [B, H, W] back.
    `radius` 0 returns the grown mask and launches no filter.  Two launches per chunk on the current stream and no
    device -> host read."""
    g = require_hip(image, "image", __name__)
    require_hip(mask, "mask", __name__)
    int_in(radius, 0, MAX_RADIUS, "radius")
    int_in(grow, -MAX_GROW, MAX_GROW, "grow")
    eps = float(eps)
    if not EPS_RANGE[0] <= eps <= EPS_RANGE[1]:
        raise ValueError(f"eps must lie in [{EPS_RANGE[0]}, {EPS_RANGE[1]}], got {eps!r}")
    B, H, W, C = image4(g, "image").shape
    if C == 2:
        raise ValueError(f"image {tuple(g.shape)}: the guide has 1 channel or at least 3")
    g = _as_f32c(g)
    dev = g.device
    m = grow_mask(mask_for(mask, B, H, W, dev), grow)
    if radius == 0:
        return m.expand(B, H, W).clone()
    parts = list(chunks(B, _cabi.refine_ws_bytes(1, H, W, C, radius), WS_CAP_BYTES))
    ws = workspace(_cabi.load().lp_refine_ws_bytes(parts[0][1], H, W, C, radius), dev, "lp_refine_ws_bytes")
    out = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    for s, n in parts:
        mc = m if m.shape[0] == 1 else m[s:s + n]
        d = _cabi.LpRefineDesc(n, H, W, C, mc.shape[0], radius, eps, g[s:s + n].data_ptr(), mc.data_ptr(),
                               out[s:s + n].data_ptr(), ws.data_ptr(), ws.numel())
        launch("lp_mask_refine", dev, ctypes.byref(d))
    return out
