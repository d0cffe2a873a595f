"""Multiband blend: put a generated image back into the original with a Laplacian-pyramid (Burt-Adelson) seam.

MaskBlend's rule, which every stitch and decode ends in, is one feather of at most 51 pixels.  A VAE round trip, an outpaint
continuation or a detailed crop never reproduces the low frequencies of the original exactly, and whatever spatially varying
difference the colour match leaves -- shading, a gradient, a vignette -- is squeezed into that one band: a narrow band shows
it as a step, a wide one ghosts fine texture.  Here every frequency band is blended over a width in proportion to its
wavelength, coarse bands wide, fine bands at the mask's edge.  Use it after any stitch or decode: stitch with blend_overlap = 1
(a hard paste), then blend original and stitched through the mask.

blend_multiband(image1, image2, mask, levels=5) -> image
        image1 is kept where the mask is 0, image2 shown where it is 1; the soft mask is used as given (W_0 = min(m, 1) for
        m > 0, else 0).  fp32, every operation rounded on its own, on the difference image D = image2 - image1:
          levels    halved, rounded up, `levels` times or until (1, 1): n levels above the image
          REDUCE    the separable 5-tap kernel (1, 4, 6, 4, 1) / 16 at stride 2, indices clamped, rows first
          EXPAND    its 2x counterpart: (1, 6, 1) / 8 at even indices, (1, 1) / 2 at odd ones, indices clamped, rows first
          collapse  R_n = W_n * D_n, R_l = EXPAND(R_{l+1}) + W_l * (D_l - EXPAND(D_{l+1})), out = image1 + R_0
        image1 == image2 comes back bit for bit whatever the mask, an all-zero mask gives image1 bit for bit, and no pixel
        further than 2^(n+2) - 4 from the mask changes (124 pixels at the default of 5 levels).  include/lanpaint_hip.h
        (lp_multiband_blend) states the rule in full.

HIP tensors only, no CPU fallback.  The batch runs in chunks whose workspace stays under WS_CAP_BYTES; frames are independent,
so chunking cannot change a bit.
"""
from __future__ import annotations

import ctypes

import torch

from . import _cabi
from ._hostcall import chunks, image4, int_in, launch, mask_for, require_hip, workspace
from ._util import _as_f32c

MAX_SIDE = _cabi.LP_DETAIL_MAX_SIDE
MAX_LEVELS = 16
WS_CAP_BYTES = 1 << 30


def blend_multiband(image1, image2, mask, levels=5):
    """`image1` where the mask is 0, `image2` where it is 1, every frequency band blended over its own width (module
    docstring).  Images [B, H, W, C], `mask` [B, H, W], [1, H, W] or [H, W].  At most 2 * levels launches per chunk on the
    current stream and no device -> host read."""
    a = image4(require_hip(image1, "image1", __name__), "image1")
    b = require_hip(image2, "image2", __name__)
    require_hip(mask, "mask", __name__)
    int_in(levels, 0, MAX_LEVELS, "levels")
    if tuple(b.shape) != tuple(a.shape):
        raise ValueError(f"image2 shape {tuple(b.shape)} does not match image1 {tuple(a.shape)}")
    a = _as_f32c(a)
    dev = a.device
    b = _as_f32c(b.to(dev))
    B, H, W, C = a.shape
    m = mask_for(mask, B, H, W, dev)
    parts = list(chunks(B, _cabi.multiband_ws_bytes(1, H, W, C, levels), WS_CAP_BYTES))
    ws = workspace(_cabi.load().lp_multiband_ws_bytes(parts[0][1], H, W, C, levels), dev, "lp_multiband_ws_bytes")
    out = torch.empty_like(a)
    for s, n in parts:
        mc = m if m.shape[0] == 1 else m[s:s + n]
        d = _cabi.LpMultibandDesc(n, H, W, C, mc.shape[0], levels, a[s:s + n].data_ptr(), b[s:s + n].data_ptr(),
                                  mc.data_ptr(), out[s:s + n].data_ptr(), ws.data_ptr(), ws.numel())
        launch("lp_multiband_blend", dev, ctypes.byref(d))
    return out
