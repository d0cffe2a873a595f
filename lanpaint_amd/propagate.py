"""Video mask propagate: one mask painted on one frame of a clip follows the picture's motion through the other frames.

The video chain could morph a mask between painted keyframes (`LanPaint_VideoMaskEditor`, which follows a subject's centroid, not
its outline), de-flicker it (`LanPaint_VideoMaskStabilize`, not motion-compensated) and snap it to image edges
(`LanPaint_MaskRefine`); every one of them takes the per-frame mask as given.  This is the first link:

    one painted mask + the video -> propagate -> stabilize -> refine -> encode / Detailer crops

propagate_masks(images, mask, key_frame=0, levels=4, search=2, smooth=8) -> mask [F, H, W]
        `images` [F, H, W, C]; `mask` [H, W], [1, H, W] or [F, H, W] (then frame `key_frame` of it is taken), binarised at 0.5.
        From the key frame outwards, one frame at a time and in both directions, a block matching weighted by the current mask
        measures the motion to the next frame on a pyramid of `levels` levels (8 x 8 blocks, +-`search` pixels around the coarser
        level's vector, `smooth` the price of a pixel of displacement, 1/16 pixel at the finest level); holes are filled from
        neighbouring blocks and the field is median-filtered.  A map of key-frame positions is carried along the motion and the key
        mask is sampled through it, so the outline follows the picture and is resampled once, however long the clip.  All of it is
        integer arithmetic: the same bits on every run; one frame returns the binarised mask, an empty mask stays exactly 0, a full
        mask exactly 1, a still video returns the binarised key mask on every frame, a noise-free whole-pixel shift is tracked
        exactly.  include/lanpaint_hip.h (lp_prop_*) states the rule in full.  Not handled: occlusion -- what leaves the
        picture or is covered does not come back.  Several keyframes, which pull drift back: propagate_keys.py.  One key matched
        against every frame again, which keeps sub-pixel drift from adding up: propagate_anchored.py.

HIP tensors only, no CPU fallback, no device -> host read.  The luma pyramids are built in chunks of frames that stay under
WS_CAP_BYTES; a frame's pyramid depends on that frame only, so chunking cannot change a bit.  A step is 2 levels + 1 launches
(a match and a fill per level, one advance), and the F - 1 steps of the two chains depend on one another in turn.
"""
from __future__ import annotations

import ctypes

import torch

from . import _cabi
from ._hostcall import chunks, int_in, launch, require_hip, tensor_is, workspace
from ._motion import (MAX_LEVELS, MAX_SEARCH, MAX_SIDE, MAX_SMOOTH, check_images, check_params, check_plane,     # noqa: F401
                      clip_mask, level_view, luma_pyramids)                    # (the limits are this module's to export, as before)
from ._util import _as_f32c

WS_CAP_BYTES = 1 << 30


def key_mask(mask, levels):
    """The key mask fp32 [H, W] binarised at 0.5: (its bits' pyramid uint8 [1, stride], the bits as fp32 [H, W]).  One launch."""
    int_in(levels, 1, MAX_LEVELS, "levels")
    require_hip(mask, "mask", __name__)
    if mask.ndim != 2:
        raise ValueError(f"the key mask must be [H, W], got {tuple(mask.shape)}")
    mask = _as_f32c(mask)
    H, W = mask.shape
    check_plane(H, W)
    mpyr = workspace(_cabi.load().lp_prop_pyramid_ws_bytes(1, H, W, levels), mask.device, "lp_prop_pyramid_ws_bytes")
    out = torch.empty((H, W), dtype=torch.float32, device=mask.device)
    launch("lp_prop_key_mask", mask.device, mask.data_ptr(), H, W, levels, mpyr.data_ptr(), out.data_ptr())
    return mpyr.view(1, -1), out


def check_match(src, tgt, mpyr, parent, H, W, levels, level, search, smooth, module):
    """The argument block of a match of one level, single or one job of a batch: the numbers first, then one frame's pyramid
    each, [stride] or [1, stride], and `parent` exactly below the top level.  The level's grid; `module` is the caller's
    __name__."""
    check_params(levels, search, smooth)
    int_in(level, 0, levels - 1, "level")
    check_plane(H, W)
    stride = _cabi.prop_pyramid_ws_bytes(1, H, W, levels)
    for t, what in ((src, "src"), (tgt, "tgt"), (mpyr, "mpyr")):
        if tensor_is(t, torch.uint8, t.shape, what, module).numel() != stride:
            raise ValueError(f"{what} holds {t.numel()} bytes, a {H}x{W} pyramid of {levels} levels {stride}")
    if (parent is None) != (level == levels - 1):
        raise ValueError("parent is given exactly below the top level")
    if parent is not None:
        tensor_is(parent, torch.int32, (*_cabi.prop_grid(H, W, level + 1), 2), "parent", module)
    return _cabi.prop_grid(H, W, level)


def match_level(src, tgt, mpyr, H, W, levels, level, search=2, smooth=8, parent=None, vec=None, valid=None):
    """The match of one level of one step: `src`, `tgt` one frame's luma pyramid each, `mpyr` the source frame's mask pyramid,
    `parent` the level above's final field (None exactly at the top level).  (vec int32 [gh, gw, 2], valid int32 [gh, gw])."""
    gh, gw = check_match(src, tgt, mpyr, parent, H, W, levels, level, search, smooth, __name__)
    dev = src.device
    vec = torch.empty((gh, gw, 2), dtype=torch.int32, device=dev) if vec is None else vec
    valid = torch.empty((gh, gw), dtype=torch.int32, device=dev) if valid is None else valid
    d = _cabi.LpPropMatchDesc(H, W, levels, level, search, smooth, src.data_ptr(), tgt.data_ptr(), mpyr.data_ptr(),
                              None if parent is None else parent.data_ptr(), vec.data_ptr(), valid.data_ptr())
    launch("lp_prop_match", dev, ctypes.byref(d))
    return vec, valid


def check_field(vec, valid, module, grid=(None, None)):
    """The argument block of a fill, single or one job of a batch: `vec` int32 [gh, gw, 2] and `valid` int32 [gh, gw], of `grid`
    where a batch's first job has set it.  (gh, gw)."""
    grid = tensor_is(vec, torch.int32, (*grid, 2), "vec", module).shape[:2]
    tensor_is(valid, torch.int32, grid, "valid", module)
    return grid


def fill_median(vec, valid, out=None):
    """Fill and median of one level's field: int32 [gh, gw, 2].  One launch."""
    gh, gw = check_field(vec, valid, __name__)
    out = torch.empty_like(vec) if out is None else out
    launch("lp_prop_fill", vec.device, vec.data_ptr(), valid.data_ptr(), gh, gw, out.data_ptr())
    return out


def check_advance(vec, pos, key_bits, levels, module, plane=(None, None)):
    """The argument block of an advance, single or one job of a batch: `levels` first, then `key_bits` uint8 [H, W] (of `plane`
    where a batch's first job has set it), `vec` level 0's field of that plane, `pos` int32 [H, W, 2] or None.  (H, W)."""
    int_in(levels, 1, MAX_LEVELS, "levels")
    require_hip(vec, "vec", module)
    H, W = tensor_is(key_bits, torch.uint8, plane, "key_bits", module).shape
    check_plane(H, W)
    tensor_is(vec, torch.int32, (*_cabi.prop_grid(H, W), 2), "vec", module)
    if pos is not None:
        tensor_is(pos, torch.int32, (H, W, 2), "pos", module)
    return H, W


def advance(vec, pos, key_bits, levels, pos_out=None, out=None, mpyr_out=None):
    """The advance of one step: `vec` level 0's final field, `pos` the source frame's positions int32 [H, W, 2] (None: the key
    frame's), `key_bits` uint8 [H, W].  (positions of t, mask of t fp32 [H, W], the pyramid of its bits uint8 [1, stride])."""
    H, W = check_advance(vec, pos, key_bits, levels, __name__)
    dev = vec.device
    pos_out = torch.empty((H, W, 2), dtype=torch.int32, device=dev) if pos_out is None else pos_out
    out = torch.empty((H, W), dtype=torch.float32, device=dev) if out is None else out
    if mpyr_out is None:
        mpyr_out = workspace(_cabi.load().lp_prop_pyramid_ws_bytes(1, H, W, levels), dev, "lp_prop_pyramid_ws_bytes").view(1, -1)
    d = _cabi.LpPropAdvanceDesc(H, W, levels, 0, vec.data_ptr(), None if pos is None else pos.data_ptr(), key_bits.data_ptr(),
                                pos_out.data_ptr(), out.data_ptr(), mpyr_out.data_ptr())
    launch("lp_prop_advance", dev, ctypes.byref(d))
    return pos_out, out, mpyr_out


class Step:
    """The buffers one chain's steps share, and one step s -> t on them: 2 levels + 1 launches, nothing allocated.  The two
    refinements of the single-key family are options, each off by default, handed in by the module that owns their stages:
        rematch  (match, *numbers): propagate_anchored's (anchor_field, anchor, smooth), or propagate_anchored_visible's
                 (gated_anchor_field, anchor, smooth, occlusion) -- the gated one when `split` is on too.  A first advance, the
                 match of the warped key against the frame, fill_median, and the advance proper along that correction: + 3.
        split    (visible_flags, occlude, occlusion), propagate_visible's: the flags, then occlude, behind the last advance: + 2.
    Scratch comes with the option that needs it.  Either: `code` and `raw_mpyr`, an advance's mask and the pyramid of its bits.
    rematch: `raw_pos`, the first advance's positions.  split: `flags`.  Both: `gated`.  The plain step has none of them."""

    def __init__(self, H, W, levels, search, smooth, dev, rematch=None, split=None):
        self.H, self.W, self.levels, self.search, self.smooth = H, W, levels, search, smooth
        self.rematch, self.split = rematch, split
        grids = [_cabi.prop_grid(H, W, lv) for lv in range(levels)]
        self.raw = [torch.empty((gh, gw, 2), dtype=torch.int32, device=dev) for gh, gw in grids]
        self.valid = [torch.empty((gh, gw), dtype=torch.int32, device=dev) for gh, gw in grids]
        self.field = [torch.empty((gh, gw, 2), dtype=torch.int32, device=dev) for gh, gw in grids]
        self.pos = [torch.empty((H, W, 2), dtype=torch.int32, device=dev) for _ in range(2)]
        stride = _cabi.prop_pyramid_ws_bytes(1, H, W, levels)
        self.mpyr = [torch.empty((1, stride), dtype=torch.uint8, device=dev) for _ in range(2)]
        if rematch or split:
            self.code = torch.empty((H, W), dtype=torch.float32, device=dev)
            self.raw_mpyr = torch.empty_like(self.mpyr[0])
        if rematch:
            self.raw_pos = torch.empty_like(self.pos[0])
        if split:
            self.flags = torch.empty(grids[0], dtype=torch.int32, device=dev)
        if rematch and split:
            self.gated = torch.empty_like(self.flags)

    def field_of(self, src, tgt, mpyr):
        """Level 0's final field of the step from the frame with pyramid `src` to the one with `tgt`, weighted by `mpyr`."""
        parent = None
        for lv in range(self.levels - 1, -1, -1):
            match_level(src, tgt, mpyr, self.H, self.W, self.levels, lv, self.search, self.smooth, parent, self.raw[lv], self.valid[lv])
            parent = fill_median(self.raw[lv], self.valid[lv], self.field[lv])
        return parent

    def chain(self, frames, key_pyr, out, hidden=None):
        """`frames`: (index into out, that frame's luma pyramid) from the key outwards, the key first; writes out[t] behind it,
        and hidden[t] when the split is on.  Which buffer serves what:
          - level 0's raw, valid and field serve the correction too: the step's own field is spent by the first advance;
          - the first advance's code and raw_mpyr are scratch once the re-match has read them: the second advance rewrites both;
          - with the split on, the last advance's mask is the code to split and its bits are raw_mpyr; occlude writes the
            pyramid of the next step's weights to self.mpyr[k], never to raw_mpyr, whose bits the flags have just been read from;
          - the key frame's luma is this chain's own copy, since the key's chunk may go; the plain step never looks at luma."""
        H, W, levels = self.H, self.W, self.levels
        match, *numbers = self.rematch or (None,)
        flags_of, occlude, occlusion = self.split or (None, None, None)
        refined = bool(match or occlude)
        gate = (self.gated,) if match and occlude else ()
        pos, mpyr, src, k, luma, key_luma = None, key_pyr, None, 0, None, None
        key_bits = level_view(key_pyr, H, W, 0)[0]
        bits = level_view(self.raw_mpyr, H, W, 0)[0] if refined else None
        for t, pyr in frames:
            if refined:
                luma = level_view(pyr[None], H, W, 0)[0]
            if src is None:
                key_luma = luma.clone() if refined else None
            else:
                vec = self.field_of(src, pyr, mpyr)
                if match:
                    advance(vec, pos, key_bits, levels, self.raw_pos, self.code, self.raw_mpyr)
                    match(self.raw_pos, luma, key_luma, bits, *numbers, self.raw[0], self.valid[0], *gate)
                    vec, pos = fill_median(self.raw[0], self.valid[0], self.field[0]), self.raw_pos
                if occlude:
                    pos, _, _ = advance(vec, pos, key_bits, levels, self.pos[k], self.code, self.raw_mpyr)
                    flags_of(pos, luma, key_luma, bits, occlusion, self.flags)
                    _, _, mpyr = occlude(self.code, self.flags, levels, out[t], hidden[t], self.mpyr[k])
                else:
                    pos, _, mpyr = advance(vec, pos, key_bits, levels, self.pos[k], out[t], self.mpyr[k])
                k ^= 1
            src = pyr


def chain_frames(images, order, levels):
    """(frame index, its luma pyramid) along `order`, the pyramids built a chunk of frames at a time under WS_CAP_BYTES."""
    F, H, W, C = images.shape
    per_frame = _cabi.prop_pyramid_ws_bytes(1, H, W, levels) + (0 if images.dtype == torch.float32 else H * W * C * 4)
    for s, n in chunks(len(order), per_frame, WS_CAP_BYTES):
        idx = order[s:s + n]
        lo, hi = min(idx), max(idx) + 1
        pyr = luma_pyramids(images[lo:hi], levels)
        for f in idx:                                                # the chunk's last frame is the next chunk's first source:
            yield f, (pyr[f - lo].clone() if f == idx[-1] else pyr[f - lo])     # its own copy lets the chunk go


def key_and_orders(images, mask, key_frame, levels):
    """What the two single-key forms start from: (the pyramid of the key mask's bits, an output fp32 [F, H, W] with the key frame
    written, the frames of the chains that have a step: forwards from the key, backwards from it).  One launch."""
    F, H, W, _ = images.shape
    mask = clip_mask(mask, F, H, W, __name__)
    key_pyr, key_out = key_mask(mask[key_frame if mask.shape[0] == F else 0].to(images.device), levels)
    out = torch.empty((F, H, W), dtype=torch.float32, device=images.device)
    out[key_frame] = key_out
    return key_pyr, out, [o for o in (list(range(key_frame, F)), list(range(key_frame, -1, -1))) if len(o) > 1]


def run(images, mask, key_frame, levels, search, smooth, rematch=None, split=None):
    """What the four single-key forms do behind their checks, `rematch` and `split` as Step takes them: the mask fp32 [F, H, W],
    and with the split (mask, hidden), the key frame's `hidden` zero."""
    key_pyr, out, orders = key_and_orders(images, mask, key_frame, levels)
    hidden = None
    if split:
        hidden = torch.empty_like(out)
        hidden[key_frame].zero_()
    step = Step(*images.shape[1:3], levels, search, smooth, images.device, rematch, split)
    for order in orders:
        step.chain(chain_frames(images, order, levels), key_pyr, out, hidden)
    return (out, hidden) if split else out


def propagate_masks(images, mask, key_frame=0, levels=4, search=2, smooth=8):
    """`mask`, painted on frame `key_frame` of `images` [F, H, W, C], followed through every frame (module docstring): fp32
    [F, H, W] on the images' device.  No device -> host read."""
    check_params(levels, search, smooth)
    check_images(images)
    require_hip(mask, "mask", __name__)
    int_in(key_frame, 0, images.shape[0] - 1, "key_frame")
    return run(images, mask, key_frame, levels, search, smooth)
