"""Masked-area fill and outpaint canvas: decide what lies under the mask before the image goes into the VAE.

The sampler ignores the latent inside the mask; the VAE encoder does not ignore the pixels there, because its receptive field
reaches across the mask's edge.  A grey border on an extended canvas, or an unwanted object under an inpaint mask, leaks into the
known latent beside the edge and comes back as a halo or a seam; with denoise < 1 it is also where the sampler starts.  Both
functions run on the device (csrc/fill_kernel.hip) and read nothing back.

fill_masked(image, mask) -> image
        Every masked pixel (mask > 0.5; a NaN is not) is replaced by a smooth continuation of the known ones, every image of the
        batch on its own, by a push-pull pyramid in fp32 with every operation rounded on its own:
          levels  (h_0, w_0) = (H, W), then halved and rounded up until (1, 1)
          pull    a coarse pixel is the mean of its known children -- s = 0, s = s + child in the order (0,0), (0,1), (1,0),
                  (1,1), then s / n -- and known when it has one
          push    from the top down, a pixel that is not known takes the 2x bilinear upsample of the level above (pixel centres
                  aligned, taps clamped, weights 0.25 / 0.75, rows first)
        Known pixels come back bit for bit; an image with no known pixel comes back unchanged; no output depends on the image
        under the mask.  include/lanpaint_hip.h (lp_mask_fill) states the rule in full.

fill_masked_patch(image, mask, radius=3, levels=AUTO, iters=4, seed=0) -> image
        The same pre-fill, then under the mask texture copied from the known part of the same image: a PatchMatch search (patches
        of 2 * radius + 1 pixels a side on 8-bit codes, `iters` Jacobi rounds of propagation and seeded random search per pyramid
        level, `levels` levels coarse to fine) and a vote that averages what the overlapping patches bring.  Where smooth
        continuation blurs grass, brick, fabric or gravel, this repeats them.  Known pixels come back bit for bit; an image with no
        hole comes back unchanged; one with no hole-free patch is fill_masked's result bit for bit; nothing depends on the image
        under the mask; the bits are the same on every run and for every batch and chunk.  include/lanpaint_hip.h (LP_FILL_PATCH)
        states the rule in full.  Not handled: smooth shading (an exemplar fill cannot extrapolate a gradient -- on a plain colour
        ramp it is worse than fill_masked, which stays the choice there); temporal coherence (frames are filled independently:
        temporal_fill goes in front, temporal_smooth behind); more than 4 channels.  The batch runs in chunks whose workspace stays
        under WS_CAP_BYTES.

plan_outpaint(H, W, left, top, right, bottom, overlap, multiple_of) -> OutpaintPlan
        The final pads and the canvas size.  Per axis with pads (p0, p1) and M = multiple_of: when the axis is padded and M > 1,
        the canvas is brought up to the next multiple of M by e = (-(p0 + N + p1)) mod M more pixels -- split e // 2 low and the
        rest high when both pads are positive, otherwise added to the one positive pad.  An unpadded axis is left alone.

outpaint_pad(image, mask=None, left=0, top=0, right=0, bottom=0, overlap=0, multiple_of=8, fill=True) -> (image, mask)
        The canvas [B, H', W', C] with the original inside and 0.0 elsewhere, and its mask [Bm, H', W'] = max(band, incoming mask):
        band is 1.0 outside the original and, inside it, within `overlap` pixels of every padded side (hard, not feathered: the
        sampler binarises at 0.5, the soft seam is blend_overlap's after the decode).  With `fill`, the canvas's masked area is
        then filled from the original by fill_masked.

HIP tensors only, no CPU fallback.
"""
from __future__ import annotations

import ctypes
import dataclasses

import torch

from . import _cabi
from ._hostcall import MAX_BATCH, chunks, image4, int_in, launch, mask_for, require_hip, workspace
from ._util import _as_f32c

MAX_SIDE = _cabi.LP_DETAIL_MAX_SIDE
AUTO = 0                              # fill_masked_patch's `levels`: as many as leave room for four patches a side
WS_CAP_BYTES = 1 << 30                # fill_masked_patch's workspace, about 28 bytes a pixel, per chunk of images


@dataclasses.dataclass(frozen=True)
class OutpaintPlan:
    left: int
    top: int
    right: int
    bottom: int
    overlap: int
    height: int      # of the canvas
    width: int


def _mask_for(mask, image, dev):
    return mask_for(require_hip(mask, "mask", __name__), image.shape[0], image.shape[1], image.shape[2], dev)


def _snap(n, p0, p1, m):
    if p0 + p1 > 0 and m > 1:
        e = (-(p0 + n + p1)) % m
        if p0 > 0 and p1 > 0:
            p0, p1 = p0 + e // 2, p1 + e - e // 2
        elif p0 > 0:
            p0 += e
        else:
            p1 += e
    return p0, p1


def plan_outpaint(H, W, left=0, top=0, right=0, bottom=0, overlap=0, multiple_of=8):
    """The final pads and the canvas size (module docstring).  ValueError: a negative value, multiple_of < 1, all four pads zero,
    an overlap that leaves no known pixel on an axis, a canvas side above the limit."""
    for v, what in ((H, "H"), (W, "W"), (multiple_of, "multiple_of")):
        int_in(v, 1, MAX_SIDE, what)             # (a multiple_of above the largest side has no canvas)
    for v, what in ((left, "left"), (top, "top"), (right, "right"), (bottom, "bottom"), (overlap, "overlap")):
        int_in(v, 0, MAX_SIDE, what)
    if left == top == right == bottom == 0:
        raise ValueError("all four pads are zero: nothing to outpaint")
    left, right = _snap(W, left, right, multiple_of)
    top, bottom = _snap(H, top, bottom, multiple_of)
    for n, p0, p1, axis in ((W, left, right, "width"), (H, top, bottom, "height")):
        if overlap * ((p0 > 0) + (p1 > 0)) >= n:
            raise ValueError(f"overlap {overlap} along every padded side leaves no known pixel of the {axis} {n}")
    height, width = top + H + bottom, left + W + right
    if max(height, width) > MAX_SIDE:
        raise ValueError(f"canvas {height} x {width} exceeds the largest side {MAX_SIDE}")
    return OutpaintPlan(left, top, right, bottom, overlap, height, width)


def fill_masked(image, mask):
    """`image` [B, H, W, C] with its masked pixels filled from the known ones (module docstring).  `mask` is [B, H, W], [1, H, W]
    or [H, W].  At most six launches on the current stream and no device -> host read."""
    img = _as_f32c(image4(require_hip(image, "image", __name__), "image", MAX_BATCH))
    dev = img.device
    m = _mask_for(mask, img, dev)
    b, h, w, c = img.shape
    ws = workspace(_cabi.load().lp_fill_ws_bytes(b, h, w, c), dev, "lp_fill_ws_bytes")
    out = torch.empty_like(img)
    d = _cabi.LpFillDesc(b, h, w, c, m.shape[0], 0, img.data_ptr(), m.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel())
    launch("lp_mask_fill", dev, ctypes.byref(d))
    return out


def patch_levels(h, w, radius):
    """AUTO: the largest L in 1..6 whose coarsest level still has min(h_{L-1}, w_{L-1}) >= 4 * (2 * radius + 1); at least 1."""
    fits = [L for L in range(1, _cabi.LP_FILL_PATCH_MAX_LEVELS + 1) if min(_cabi.fill_patch_levels(h, w, L)[-1]) >= 4 * (2 * radius + 1)]
    return max(fits, default=1)


def fill_masked_patch(image, mask, radius=3, levels=AUTO, iters=4, seed=0):
    """`image` [B, H, W, C], C <= 4, with its masked pixels filled with texture from the known ones (module docstring).  `mask` is
    [B, H, W], [1, H, W] or [H, W].  One lp_mask_fill call per chunk of images on the current stream and no device -> host read."""
    img = image4(require_hip(image, "image", __name__), "image")
    int_in(radius, 1, _cabi.LP_FILL_PATCH_MAX_RADIUS, "radius")
    int_in(levels, AUTO, _cabi.LP_FILL_PATCH_MAX_LEVELS, "levels")
    int_in(iters, 1, _cabi.LP_FILL_PATCH_MAX_ITERS, "iters")
    int_in(seed, 0, 65535, "seed")
    if img.shape[3] > _cabi.LP_FILL_PATCH_MAX_CHANNELS:
        raise ValueError(f"image {tuple(img.shape)}: the patch fill takes at most {_cabi.LP_FILL_PATCH_MAX_CHANNELS} channels")
    img = _as_f32c(img)
    dev = img.device
    m = _mask_for(mask, img, dev)
    b, h, w, c = img.shape
    L = levels if levels != AUTO else patch_levels(h, w, radius)
    mode = _cabi.LP_FILL_PATCH(radius, L, iters, seed)
    parts = list(chunks(b, _cabi.fill_patch_ws_bytes(1, h, w, c, L), WS_CAP_BYTES))
    ws = workspace(_cabi.fill_patch_ws_bytes(parts[0][1], h, w, c, L), dev)
    out = torch.empty_like(img)
    for s, n in parts:
        mc = m if m.shape[0] == 1 else m[s:s + n]
        d = _cabi.LpFillDesc(n, h, w, c, mc.shape[0], mode, img[s:s + n].data_ptr(), mc.data_ptr(), out[s:s + n].data_ptr(),
                             ws.data_ptr(), ws.numel())
        launch("lp_mask_fill", dev, ctypes.byref(d))
    return out


def outpaint_pad(image, mask=None, left=0, top=0, right=0, bottom=0, overlap=0, multiple_of=8, fill=True):
    """(canvas [B, H', W', C], mask [Bm, H', W']) on the device (module docstring); the pads are plan_outpaint's."""
    img = image4(require_hip(image, "image", __name__), "image", MAX_BATCH)
    b, h, w, c = img.shape
    plan = plan_outpaint(h, w, left, top, right, bottom, overlap, multiple_of)
    img = _as_f32c(img)
    dev = img.device
    m = _mask_for(mask, img, dev) if mask is not None else None
    canvas = torch.empty((b, plan.height, plan.width, c), dtype=torch.float32, device=dev)
    mask_out = torch.empty((m.shape[0] if m is not None else 1, plan.height, plan.width), dtype=torch.float32, device=dev)
    d = _cabi.LpOutpaintDesc(b, h, w, c, m.shape[0] if m is not None else 0, plan.left, plan.top, plan.right, plan.bottom,
                             plan.overlap, 0, img.data_ptr(), m.data_ptr() if m is not None else None, canvas.data_ptr(),
                             mask_out.data_ptr())
    launch("lp_outpaint_pad", dev, ctypes.byref(d))
    if fill:
        canvas = fill_masked(canvas, mask_out)
    return canvas, mask_out
