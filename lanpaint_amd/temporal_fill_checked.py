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
from ._hostcall import int_in, launch
from ._motion import check_images, check_params

DISPUTED = _cabi.LP_TFILL_DISPUTED
MAX_AGREE = 255


def carry_pair(vec, known, donor_known, state, images, filled, source, remaining, witnesses, frame, reach=0, agree=8, out=None):
    """The backward step of the checked form for frame `frame`, its donor `frame + 1`: `temporal_fill.carry`'s planes, with
    `filled` and `source` as the forward pass left them, and `witnesses` int32 [F, H, W], whose plane `frame` is written.  The
    frame's (org, pos), `out` when given.  One launch."""
    int_in(reach, 0, _tf.MAX_REACH, "reach")
    int_in(agree, 1, MAX_AGREE, "agree")
    F, H, W, C = check_images(images).shape
    int_in(F, 2, _tf.MAX_FRAMES, "the frame count")
    int_in(frame, 0, F - 2, "frame")
    out = _tf.carry_planes(vec, known, donor_known, state, images, filled, source, remaining, out, witnesses=witnesses)
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
    check_params(levels, search, smooth)
    int_in(reach, 0, _tf.MAX_REACH, "reach")
    int_in(agree, 1, MAX_AGREE, "agree")
    images, filled, remaining, source, pyramids = _tf.clip_outputs(images, mask, levels)
    F, H, W, C = images.shape
    witnesses = torch.empty((F, H, W), dtype=torch.int32, device=images.device)
    if F == 1:
        return filled, remaining, source, witnesses.zero_()
    states = [_tf.new_state(H, W, images.device) for _ in range(2)]
    ptrs = (images.data_ptr(), filled.data_ptr(), source.data_ptr(), remaining.data_ptr())
    forward = _cabi.LpTfillCarryDesc(F, H, W, C, 0, 0, reach, 0, None, None, None, None, None, None, None, *ptrs)
    backward = _cabi.LpTfillCarryPairDesc(F, H, W, C, 0, 0, reach, agree, None, None, None, None, None, None, None, *ptrs,
                                          witnesses.data_ptr())
    fields_args = (H, W, levels, search, smooth)
    _tf.carry_direction("lp_tfill_carry", forward, list(range(F)), pyramids, states, fields_args, _tf.WS_CAP_BYTES)
    last = source[F - 1]                                                 # the last frame has no backward step: A alone counts
    witnesses[F - 1] = ((last >= 0) & (last != F - 1)).to(torch.int32)
    _tf.carry_direction("lp_tfill_carry_pair", backward, list(range(F - 1, -1, -1)), pyramids, states, fields_args, _tf.WS_CAP_BYTES)
    return filled, remaining, source, witnesses
