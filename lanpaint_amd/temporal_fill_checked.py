"""Checked video temporal fill: `temporal_fill` with a consistency check on what is borrowed.

`temporal_fill` believes the one-layer background field everywhere.  When something other than the masked subject moves through
the hole, it pastes the wrong picture with confidence; that picture then passes the encode as "known" and the sampler never
repaints it.  A wrong known pixel is worse than a pixel left in `remaining`.  Here the two directions of the carry are witnesses
of one another: where the forward and the backward pass both have an origin for a masked pixel, both are sampled, and per 8 x 8
block the mean absolute difference of their lumas, a brightness bias forgiven, is held against `agree`.  A block that disagrees is
a dispute: it is left to the sampler.

temporal_fill_checked(images, mask, levels=4, search=2, smooth=8, reach=0, agree=8) -> (filled, remaining, source, witnesses)
        The arguments of `temporal_fill`, and `agree` in 1..255, the mean luma residual in grey levels above which a block is
        disputed.  `filled`, `remaining`, `source` as there, except under a dispute: `filled` keeps the images, `remaining` is 1.0
        and `source` is -2 (DISPUTED).  `witnesses` int32 [F, H, W]: 2 where both directions had an origin and the block had
        pixels enough (16) to be tested and agreed, 1 where one direction vouches alone or the block was too small to test, 0
        under a dispute, where nothing was found and outside the mask.  Wherever `source` is not -2 the three outputs carry the
        bits of `temporal_fill` on the same arguments; where it is -2 the plain call had borrowed.  The last frame has no backward
        step, so its borrowed pixels have one witness.  include/lanpaint_hip.h (lp_tfill_carry_pair) states the rule in full.
        Not done: colour or exposure matching of what is borrowed (DetailerColorMatch exists), motion boundaries finer than a
        block; a wrong pixel that only one direction reaches is not caught -- `witnesses == 2` excludes those.

HIP tensors only, no CPU fallback, no device -> host read.  The pyramids, the fields, the forward carries and the chunking under
temporal_fill.WS_CAP_BYTES are `temporal_fill`'s; the backward carries are lp_tfill_carry_pair, one launch per step.
"""
from __future__ import annotations

import ctypes

import torch

from . import _cabi
from . import temporal_fill as _tf
from ._hostcall import chunks, int_in, launch, require_hip
from ._util import _as_f32c
from .propagate import _images, _params

DISPUTED = _cabi.LP_TFILL_DISPUTED
MAX_AGREE = 255


def carry_pair(vec, known, donor_known, state, images, filled, source, remaining, witnesses, frame, reach=0, agree=8, out=None):
    """The backward step of the checked form for frame `frame`, its donor `frame + 1`: `temporal_fill.carry`'s planes, with
    `filled` and `source` as the forward pass left them, and `witnesses` int32 [F, H, W], whose plane `frame` is written.  The
    frame's (org, pos), `out` when given.  One launch."""
    int_in(reach, 0, _tf.MAX_REACH, "reach")
    int_in(agree, 1, MAX_AGREE, "agree")
    images = _images(images)
    F, H, W, C = images.shape
    int_in(F, 2, _tf.MAX_FRAMES, "the frame count")
    int_in(frame, 0, F - 2, "frame")
    out = _tf.new_state(H, W, images.device) if out is None else out
    planes = [(vec, torch.int32, (*_cabi.prop_grid(H, W), 2), "vec"), (known, torch.uint8, (H, W), "known"),
              (donor_known, torch.uint8, (H, W), "donor_known"), (images, torch.float32, (F, H, W, C), "images"),
              (filled, torch.float32, (F, H, W, C), "filled"), (source, torch.int32, (F, H, W), "source"),
              (remaining, torch.float32, (F, H, W), "remaining"), (witnesses, torch.int32, (F, H, W), "witnesses"),
              (out[0], torch.int32, (H, W), "the state's org"), (out[1], torch.int32, (H, W, 2), "the state's pos")]
    if state is not None:
        planes += [(state[0], torch.int32, (H, W), "the donor state's org"), (state[1], torch.int32, (H, W, 2), "the donor state's pos")]
    for t, dtype, shape, what in planes:
        if require_hip(t, what, __name__).dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
            raise ValueError(f"{what} must be a contiguous {dtype} {list(shape)}, got {t.dtype} {list(t.shape)}")
    d = _cabi.LpTfillCarryPairDesc(F, H, W, C, frame, frame + 1, reach, agree, vec.data_ptr(), known.data_ptr(),
                                   donor_known.data_ptr(), None if state is None else state[0].data_ptr(),
                                   None if state is None else state[1].data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                                   images.data_ptr(), filled.data_ptr(), source.data_ptr(), remaining.data_ptr(),
                                   witnesses.data_ptr())
    launch("lp_tfill_carry_pair", images.device, ctypes.byref(d))
    return out


def temporal_fill_checked(images, mask, levels=4, search=2, smooth=8, reach=0, agree=8):
    """`temporal_fill` with the two directions as witnesses of one another (module docstring): (filled fp32 [F, H, W, C],
    remaining fp32 [F, H, W], source int32 [F, H, W], witnesses int32 [F, H, W]) on the images' device.  No device -> host
    read."""
    _params(levels, search, smooth)
    int_in(reach, 0, _tf.MAX_REACH, "reach")
    int_in(agree, 1, MAX_AGREE, "agree")
    _images(images)
    F, H, W, C = images.shape
    int_in(F, 1, _tf.MAX_FRAMES, "the frame count")
    dev = images.device
    mask = _as_f32c(_tf._mask3(mask, F, H, W).to(dev))
    images = _as_f32c(images)
    filled = images.clone()
    source = torch.empty((F, H, W), dtype=torch.int32, device=dev)
    remaining = torch.empty((F, H, W), dtype=torch.float32, device=dev)
    witnesses = torch.empty((F, H, W), dtype=torch.int32, device=dev)
    pyramids = _tf._Pyramids(images, mask, levels, source, remaining)
    if F == 1:
        pyramids.get(0, 1)                                               # source and remaining of the one frame
        return filled, remaining, source, witnesses.zero_()
    stride = _cabi.prop_pyramid_ws_bytes(1, H, W, levels)
    gh, gw = _cabi.prop_grid(H, W)
    per_step = 2 * stride + gh * gw * 8
    states = [_tf.new_state(H, W, dev) for _ in range(2)]
    ptrs = (images.data_ptr(), filled.data_ptr(), source.data_ptr(), remaining.data_ptr())
    forward = _cabi.LpTfillCarryDesc(F, H, W, C, 0, 0, reach, 0, None, None, None, None, None, None, None, *ptrs)
    backward = _cabi.LpTfillCarryPairDesc(F, H, W, C, 0, 0, reach, agree, None, None, None, None, None, None, None, *ptrs,
                                          witnesses.data_ptr())
    for entry, desc, order in (("lp_tfill_carry", forward, list(range(F))), ("lp_tfill_carry_pair", backward, list(range(F - 1, -1, -1)))):
        if desc is backward:                                             # the last frame has no backward step: A alone counts
            last = source[F - 1]
            witnesses[F - 1] = ((last >= 0) & (last != F - 1)).to(torch.int32)
        done = 0                                                         # carries of this direction so far
        for first, n in chunks(F - 1, per_step, max(_tf.WS_CAP_BYTES - 2 * stride, 1)):
            lo, hi = min(order[first], order[first + n]), max(order[first], order[first + n]) + 1
            luma, known = pyramids.get(lo, hi)
            fields = _tf.step_fields(luma, known, [(order[k] - lo, order[k - 1] - lo) for k in range(first + 1, first + n + 1)],
                                     H, W, levels, search, smooth)
            for j, k in enumerate(range(first + 1, first + n + 1)):
                t, s = order[k], order[k - 1]
                src, dst = states[(done + 1) & 1], states[done & 1]
                desc.frame, desc.donor, desc.vec = t, s, fields[j].data_ptr()
                desc.known, desc.donor_known = known[t - lo].data_ptr(), known[s - lo].data_ptr()
                desc.org_src, desc.pos_src = (None, None) if done == 0 else (src[0].data_ptr(), src[1].data_ptr())
                desc.org_dst, desc.pos_dst = dst[0].data_ptr(), dst[1].data_ptr()
                launch(entry, dev, ctypes.byref(desc))
                done += 1
    return filled, remaining, source, witnesses
