"""Video mask propagate, occlusion-aware: the carried mask stays off whatever passes in front of the subject.

`propagate.propagate_masks` carries one painted mask along the picture's motion; when the subject passes behind a lamp post, that
mask lies on the post and the sampler repaints the post.  Nothing downstream repairs it: the stabilize is not motion-compensated,
the refine only snaps edges, the Detailer crops take the mask as given.  The position map every step carries names, for each pixel
of frame t, where it was in the key frame; the key frame's luma sampled through it shows what the subject should look like there.
Where the picture of t looks different, something is in front.

propagate_masks_visible(images, mask, key_frame=0, levels=4, search=2, smooth=8, occlusion=16) -> (mask [F, H, W], hidden [F, H, W])
        The single-key chain with two launches behind every advance.  lp_prop_visible: per 8 x 8 block, over the mask pixels of the
        block's 16 x 16 window, the mean absolute difference between the frame's luma and the warped key luma, after a brightness
        bias of at most 32 grey levels is forgiven; above `occlusion` grey levels the block counts as occluded.  lp_prop_occlude:
        the flags, interpolated between block centres, split the carried mask code c into the visible part c' (`mask`, which also
        gives the bits that weight the next step's match) and the rest (`hidden`, the part of the subject behind something; add it
        back to inpaint through the occluder).  Nothing is remembered between frames: the test is against the key frame every
        time, so what was hidden is visible again as soon as it looks like the key again, and the hidden part's positions follow
        the visible rest (blocks without bits are filled from their neighbours).  The key frame returns its binarised mask and a
        zero `hidden`.  occlusion = 0 switches the test off: propagate_masks and zeros, no further launch.
        Integer arithmetic throughout: a still video and a noise-free whole-pixel shift return the binarised key mask and a zero
        `hidden`; an empty mask gives 0 and 0.  include/lanpaint_hip.h (lp_prop_visible, lp_prop_occlude) states the rule in full.
        Not handled: a subject that is hidden entirely leaves the zero field and is lost if it reappears elsewhere; what leaves
        the picture; occlusion edges finer than a block -- `LanPaint_MaskRefine` follows in the chain.  Several keyframes with
        occlusion, where a second key behind the occluder recovers a lost subject: propagate_keys_visible.py.  A lower `occlusion` hides more and starts to take sub-pixel motion and noise
        for an occluder; profiles/r29_propagate_visible.md has the numbers behind the default.  On a long clip with sub-pixel
        motion the carried positions drift, drift reads as occlusion and the subject is lost; the form that re-matches the key
        frame first: propagate_anchored_visible.py.

HIP tensors only, no CPU fallback, no device -> host read.  The frames' luma pyramids come in propagate's chunks, under
propagate.WS_CAP_BYTES; the key frame's luma plane is copied once per chain, so it outlives its chunk.  A step is 2 levels + 3
launches and allocates nothing.
"""
from __future__ import annotations

import ctypes

import torch

from . import _cabi, propagate
from ._hostcall import int_in, launch, require_hip, tensor_is
from ._motion import check_frame_planes, check_images, check_params, check_plane
from .propagate import Step                                          # noqa: F401  (the family's one step, options and all)

MAX_OCCLUSION = 255
DEFAULT_OCCLUSION = 16


def visible_flags(pos, tgt, key, mask_bits, occlusion=DEFAULT_OCCLUSION, out=None):
    """One occlusion flag per level-0 block of frame t: `pos` its positions int32 [H, W, 2], `tgt` and `key` level 0 of its and of
    the key frame's luma pyramid, `mask_bits` level 0 of the pyramid the advance wrote, all uint8 [H, W].  int32 [gh, gw], 1 where
    the block is occluded.  One launch."""
    int_in(occlusion, 1, MAX_OCCLUSION, "occlusion")
    H, W = check_frame_planes(pos, tgt, key, mask_bits, __name__)
    out = torch.empty(_cabi.prop_grid(H, W), dtype=torch.int32, device=tgt.device) if out is None else out
    d = _cabi.LpPropVisibleDesc(H, W, occlusion, 0, pos.data_ptr(), tgt.data_ptr(), key.data_ptr(), mask_bits.data_ptr(), out.data_ptr())
    launch("lp_prop_visible", tgt.device, ctypes.byref(d))
    return out


def check_occlude(code, flags, levels, module, plane=(None, None)):
    """The argument block of an occlude, single or one job of a batch: `levels` first, then `code` fp32 [H, W] (of `plane` where
    a batch's first job has set it) and `flags` int32 on its level-0 grid.  (H, W); `module` is the caller's __name__."""
    int_in(levels, 1, propagate.MAX_LEVELS, "levels")
    H, W = tensor_is(code, torch.float32, plane, "code", module).shape
    check_plane(H, W)
    tensor_is(flags, torch.int32, _cabi.prop_grid(H, W), "flags", module)
    return H, W


def occlude(code, flags, levels, out=None, hidden=None, mpyr_out=None):
    """The advance's mask `code` fp32 [H, W] (c / 256) split by the blocks' `flags` int32 [gh, gw]: (the visible part, the hidden
    part, both fp32 [H, W], and the pyramid of the visible part's bits uint8 [1, stride]).  One launch."""
    H, W = check_occlude(code, flags, levels, __name__)
    dev = code.device
    out = torch.empty((H, W), dtype=torch.float32, device=dev) if out is None else out
    hidden = torch.empty((H, W), dtype=torch.float32, device=dev) if hidden is None else hidden
    if mpyr_out is None:
        mpyr_out = torch.empty((1, _cabi.prop_pyramid_ws_bytes(1, H, W, levels)), dtype=torch.uint8, device=dev)
    d = _cabi.LpPropOccludeDesc(H, W, levels, 0, code.data_ptr(), flags.data_ptr(), out.data_ptr(), hidden.data_ptr(),
                                mpyr_out.data_ptr())
    launch("lp_prop_occlude", dev, ctypes.byref(d))
    return out, hidden, mpyr_out


def propagate_masks_visible(images, mask, key_frame=0, levels=4, search=2, smooth=8, occlusion=DEFAULT_OCCLUSION):
    """`mask`, painted on frame `key_frame` of `images` [F, H, W, C], followed through every frame and kept off what passes in
    front of it (module docstring): (mask, hidden), fp32 [F, H, W] each, on the images' device.  No device -> host read."""
    check_params(levels, search, smooth)
    int_in(occlusion, 0, MAX_OCCLUSION, "occlusion")
    check_images(images)
    require_hip(mask, "mask", __name__)
    F, H, W, _ = images.shape
    int_in(key_frame, 0, F - 1, "key_frame")
    if occlusion == 0:
        return propagate.propagate_masks(images, mask, key_frame, levels, search, smooth), images.new_zeros((F, H, W), dtype=torch.float32)
    return propagate.run(images, mask, key_frame, levels, search, smooth, split=(visible_flags, occlude, occlusion))
