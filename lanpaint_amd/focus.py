"""Focus match: soften what was generated under the mask until its edges are as soft as the footage around it.

The finishing chain matches colour (detail_color), seam (multiband), grain (grain) and time (temporal_smooth); this is focus.  What a
decoder returns under the mask is as sharp as the model draws, a Detailer crop resampled down sharper still, while the footage around
it is as soft as the lens, the focus pull, the motion blur, the codec or an earlier upscale left it: on a soft shot the inpainted
area reads as a sticker.  Its place is behind the stitch or decode and the temporal smooth and in front of the multiband blend and the
grain match -- blur removes grain, so grain goes back after it.

match_focus(image, mask, reference=None, strength=1.0, edge=8, ring=2, per_frame=False) -> image
        `image` [B, H, W, C] is the picture to correct, `reference` (default: `image` itself) where the surroundings' sharpness is
        read -- the untouched original when there is one.  The edge blur is measured as a variance in px^2 from the ratio of the
        gradient energies of the 8-bit luma at two binomial scales (variance 0.5 and 2), over the pixels whose gradient at the
        coarse scale reaches `edge` grey levels per pixel: INSIDE where the whole 11 x 11 support is masked (> 0.5), read on
        `image`, and in a RING of `ring` 32 x 32 tiles around the tiles that hold mask, where none of the support is masked, read on
        `reference`.  v = strength * max(0, var_ring - var_inside), at most 16 px^2, in thirty-seconds; `image` is blurred under the
        soft mask with a binomial kernel of exactly that variance: out = image + m * (blur - image).  One variance for the whole
        batch (a clip), or one per image with per_frame.  include/lanpaint_hip.h ("the focus form") states the rule in full;
        integers up to the fit, so the same bits on every run.
        Bit for bit `image`: an all-zero mask, a masked area as soft as or softer than its surroundings, fewer than 64 edge pixels on
        either side, a side under 11 pixels; and nothing further than 33 pixels from the mask changes.
        NOT handled: sharpening (a generated side softer than the ring is left alone), focus that varies across the mask (one
        variance per frame or clip), textures without edges (nothing is measured, nothing happens).
focus_report(...) -> {"var_ring", "var_inside", "K"}: the device tensors of what was measured, fp64 [B], fp64 [B], int32 [B]; a side
        that fitted nothing reports NO_FIT (-1).  sqrt(K / 32) is the sigma of the blur applied.

HIP tensors only, no CPU fallback: the C entry is lp_multiband_blend with levels = LP_MULTIBAND_FOCUS(...) (five launches, no device
-> host read, torch's current stream).  per_frame runs in chunks whose workspace stays under WS_CAP_BYTES; frames are independent
there, so chunking cannot change a bit.  The pooled form measures the whole clip in one call: a clip whose workspace (4 bytes per
element of the clip, little more) exceeds WS_CAP_BYTES is refused rather than measured in parts, which would change bits.
"""
from __future__ import annotations

import ctypes

import torch

from . import _cabi
from ._hostcall import chunks, float_in, image4, int_in, launch, mask_for, require_hip, workspace
from ._util import _as_f32c

WS_CAP_BYTES = 1 << 30
MAX_POOLED_PIXELS = 1 << 30
NO_FIT = _cabi.LP_FOCUS_NO_FIT


def _run(image, mask, reference, strength, edge, ring, per_frame, report):
    a = image4(require_hip(image, "image", __name__), "image")
    require_hip(mask, "mask", __name__)
    ref = a if reference is None else require_hip(reference, "reference", __name__)
    s16 = int(float_in(strength, 0.0, 1.0, "strength") * 16.0 + 0.5)
    int_in(edge, 1, 255, "edge")
    int_in(ring, 1, _cabi.LP_FOCUS_MAX_RING, "ring")
    if not isinstance(per_frame, (bool, int)) or per_frame not in (0, 1):
        raise ValueError(f"per_frame must be a bool, got {per_frame!r}")
    if tuple(ref.shape) != tuple(a.shape):
        raise ValueError(f"reference shape {tuple(ref.shape)} does not match image {tuple(a.shape)}")
    same = ref is a
    a = _as_f32c(a)
    dev = a.device
    ref = a if same else _as_f32c(ref.to(dev))
    B, H, W, C = a.shape
    m = mask_for(mask, B, H, W, dev)
    word = _cabi.LP_MULTIBAND_FOCUS(edge, ring, s16, int(bool(per_frame)))
    if per_frame:
        parts = list(chunks(B, _cabi.focus_ws_bytes(1, H, W, C), WS_CAP_BYTES))
    else:
        if B > 65535 or B * H * W > MAX_POOLED_PIXELS or _cabi.focus_ws_bytes(B, H, W, C) > WS_CAP_BYTES:
            raise ValueError(f"a clip of {B} x {H} x {W} x {C} is measured as one and does not fit one call (workspace "
                             f"{_cabi.focus_ws_bytes(B, H, W, C)} bytes, the limit is {WS_CAP_BYTES}); measuring it in parts would "
                             "change the result: pass per_frame=True or a shorter clip")
        parts = [(0, B)]
    n0 = parts[0][1]
    ws = workspace(_cabi.load().lp_multiband_ws_bytes(n0, H, W, C, word), dev, "lp_multiband_ws_bytes")
    out = torch.empty_like(a)
    var = torch.empty((B, 2), dtype=torch.float64, device=dev) if report else None
    K = torch.empty((B,), dtype=torch.int32, device=dev) if report else None
    for s, n in parts:
        mc = m if m.shape[0] == 1 else m[s:s + n]
        d = _cabi.LpMultibandDesc(n, H, W, C, mc.shape[0], word, a[s:s + n].data_ptr(), ref[s:s + n].data_ptr(),
                                  mc.data_ptr(), out[s:s + n].data_ptr(), ws.data_ptr(), ws.numel())
        launch("lp_multiband_blend", dev, ctypes.byref(d))
        if report:
            at = _cabi.focus_ws_layout(n, H, W, C)
            var[s:s + n] = ws[at["var"]:at["var"] + 16 * n].view(torch.float64).view(n, 2)
            K[s:s + n] = ws[at["K"]:at["K"] + 4 * n].view(torch.int32)
    return out, var, K


def match_focus(image, mask, reference=None, strength=1.0, edge=8, ring=2, per_frame=False):
    """`image` blurred under `mask` by the edge softness its surroundings have and it lacks (module docstring).  Images
    [B, H, W, C], `mask` [B, H, W], [1, H, W] or [H, W]; fp32 [B, H, W, C] comes back.  Five launches per chunk on the current
    stream and no device -> host read."""
    return _run(image, mask, reference, strength, edge, ring, per_frame, False)[0]


def focus_report(image, mask, reference=None, strength=1.0, edge=8, ring=2, per_frame=False):
    """What match_focus measures with the same arguments, as device tensors: {"var_ring": fp64 [B], "var_inside": fp64 [B] (px^2,
    NO_FIT for a side with too few edge pixels), "K": int32 [B] (the variance applied, in thirty-seconds of a px^2), "image": the
    result}.  Pooled, every row holds the clip's figures."""
    out, var, K = _run(image, mask, reference, strength, edge, ring, per_frame, True)
    return {"var_ring": var[:, 0], "var_inside": var[:, 1], "K": K, "image": out}
