"""Video mask propagate from several keyframes: every painted key follows the picture's motion in both directions, and between
two keys the two carried masks are merged through their signed distance fields.

`propagate.propagate_masks` carries one key through the clip and loses accuracy with the distance from it; the video mask editor
morphs between painted keys but does not follow the picture.  This joins the two:

propagate_keys(images, masks, key_frames, levels=4, search=2, smooth=8) -> mask [F, H, W]
        `images` [F, H, W, C]; `key_frames` strictly increasing frame indices; `masks` [K, H, W] (the k-th mask belongs to the
        k-th key), [F, H, W] (the frames at the keys are read) or [H, W] for one key.  Every chain is the chain of
        `propagate_masks` started from one key (`chain_plan` lists them).  A key frame returns its binarised painted mask, a
        frame in front of the first or behind the last key its one chain's output, a frame between two keys a and b the merge:
        the signed distances of the two chains' masks, capped at 64 pixels, weighted (b - t) : (t - a), a ramp of half a pixel
        around their zero crossing.  So drift is pulled back to zero at every key.  One key gives `propagate_masks` bit for bit;
        a still video with the same mask on every key returns that binarised mask; empty stays exactly 0, full exactly 1.  An
        empty key next to a non-empty one says "nothing here": the other key's mask appears only in the last frames before it.
        include/lanpaint_hip.h (lp_prop_*_batch, lp_prop_merge) states the rule in full.  Not handled: occlusion; several
        keyframes with occlusion are propagate_keys_visible.py's, which builds on this module's chains.

HIP tensors only, no CPU fallback, no device -> host read.  The up to 2 K chains do not depend on one another, so step s of all
of them is one batch: 2 levels + 1 launches per 32 active chains, and the call has as many dependent steps as its longest chain.
The luma pyramids of the whole clip are held at once (uint8, about 4/3 byte per pixel; they must fit WS_CAP_BYTES); the fp32
conversion of other input goes in chunks under WS_CAP_BYTES.  The step loop allocates nothing: the job tables are host arrays
whose addresses move with the step.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _cabi, stabilize
from ._hostcall import int_in, launch, require_hip, tensor_is
from ._motion import MAX_JOBS, FieldWalk, check_images, check_params, check_plane, luma_pyramids, row_addresses
from .propagate import key_mask

WS_CAP_BYTES = 1 << 30


def chain_plan(frames, key_frames):
    """The chains of a clip of `frames` frames with keys `key_frames`, as (key index, key frame, direction, length): backward
    from the first key, per gap forward from its left key and backward from its right key, forward from the last key.  Step s
    of a call runs the chains with length >= s, in this order, in launches of at most LP_PROP_MAX_JOBS.  No device."""
    int_in(frames, 1, 1 << 30, "frames")
    try:
        keys = list(key_frames)
    except TypeError:
        raise ValueError(f"key_frames must be a sequence of frame indices, got {key_frames!r}") from None
    if not keys:
        raise ValueError("key_frames is empty: at least one key frame")
    for k in keys:
        int_in(k, 0, frames - 1, "a key frame")
    if any(b <= a for a, b in zip(keys, keys[1:])):
        raise ValueError(f"key_frames must be strictly increasing, got {keys}")
    plan = [(0, keys[0], -1, keys[0])]
    for i, (a, b) in enumerate(zip(keys, keys[1:])):
        plan += [(i, a, 1, b - a - 1), (i + 1, b, -1, b - a - 1)]
    plan.append((len(keys) - 1, keys[-1], 1, frames - 1 - keys[-1]))
    return [c for c in plan if c[3] > 0]


def job_table(rows, what):
    """`rows`: per job a tuple of tensors (or None); the tensors' addresses as a host uint64 [jobs, fields]."""
    if not 1 <= len(rows) <= MAX_JOBS:
        raise ValueError(f"{what}: 1..{MAX_JOBS} jobs, got {len(rows)}")
    return np.array([[0 if t is None else t.data_ptr() for t in row] for row in rows], dtype=np.uint64)


def match_level_batch(jobs, H, W, levels, level, search=2, smooth=8):
    """`propagate.match_level` for several independent steps in one launch.  `jobs`: per job (src, tgt, mpyr, parent) as there,
    `parent` None exactly at the top level.  A list of (vec int32 [gh, gw, 2], valid int32 [gh, gw])."""
    check_params(levels, search, smooth)
    int_in(level, 0, levels - 1, "level")
    check_plane(H, W)
    stride = _cabi.prop_pyramid_ws_bytes(1, H, W, levels)
    gh, gw = _cabi.prop_grid(H, W, level)
    rows, outs = [], []
    for src, tgt, mpyr, parent in jobs:
        for t, what in ((src, "src"), (tgt, "tgt"), (mpyr, "mpyr")):
            if tensor_is(t, torch.uint8, t.shape, what, __name__).numel() != stride:
                raise ValueError(f"{what} must be one frame's pyramid: {stride} contiguous uint8")
        if (parent is None) != (level == levels - 1):
            raise ValueError("parent is given exactly below the top level")
        if parent is not None:
            tensor_is(parent, torch.int32, (*_cabi.prop_grid(H, W, level + 1), 2), "parent", __name__)
        vec = torch.empty((gh, gw, 2), dtype=torch.int32, device=src.device)
        valid = torch.empty((gh, gw), dtype=torch.int32, device=src.device)
        rows.append((src, tgt, mpyr, parent, vec, valid))
        outs.append((vec, valid))
    table = job_table(rows, "match_level_batch")
    d = _cabi.LpPropMatchBatchDesc(H, W, levels, level, search, smooth, len(rows), 0, table.ctypes.data)
    launch("lp_prop_match_batch", rows[0][0].device, ctypes.byref(d))
    return outs


def fill_median_batch(jobs):
    """`propagate.fill_median` for several fields of one grid in one launch.  `jobs`: per job (vec, valid).  A list of fields."""
    rows = []
    for vec, valid in jobs:
        require_hip(vec, "vec", __name__)
        grid = tuple(rows[0][0].shape[:2] if rows else vec.shape[:2])    # the first job's grid is every job's
        tensor_is(vec, torch.int32, (*grid, 2), "vec", __name__)
        tensor_is(valid, torch.int32, grid, "valid", __name__)
        rows.append((vec, valid, torch.empty_like(vec)))
    table = job_table(rows, "fill_median_batch")
    gh, gw = rows[0][0].shape[:2]
    launch("lp_prop_fill_batch", rows[0][0].device, table.ctypes.data, len(rows), gh, gw)
    return [r[2] for r in rows]


def advance_batch(jobs, levels):
    """`propagate.advance` for several independent steps of one plane in one launch.  `jobs`: per job (vec, pos, key_bits), `pos`
    None for the key frame's positions.  A list of (positions, mask fp32 [H, W], the pyramid of its bits uint8 [1, stride])."""
    int_in(levels, 1, _cabi.LP_PROP_MAX_LEVELS, "levels")
    rows, outs = [], []
    for vec, pos, key_bits in jobs:
        require_hip(vec, "vec", __name__)
        H, W = tensor_is(key_bits, torch.uint8, rows[0][2].shape if rows else (None, None), "key_bits", __name__).shape   # one plane
        check_plane(H, W)
        tensor_is(vec, torch.int32, (*_cabi.prop_grid(H, W), 2), "vec", __name__)
        if pos is not None:
            tensor_is(pos, torch.int32, (H, W, 2), "pos", __name__)
        dev = vec.device
        new = (torch.empty((H, W, 2), dtype=torch.int32, device=dev), torch.empty((H, W), dtype=torch.float32, device=dev),
               torch.empty((1, _cabi.prop_pyramid_ws_bytes(1, H, W, levels)), dtype=torch.uint8, device=dev))
        rows.append((vec, pos, key_bits, *new))
        outs.append(new)
    table = job_table(rows, "advance_batch")
    H, W = rows[0][2].shape
    d = _cabi.LpPropAdvanceBatchDesc(H, W, levels, len(rows), table.ctypes.data)
    launch("lp_prop_advance_batch", rows[0][0].device, ctypes.byref(d))
    return outs


def merge_gap(qa, qb, span, first=1, out=None):
    """The merge of one gap's in-between frames: `qa`, `qb` int32 [n, H, W], the signed squared distances (stabilize.signed_d2)
    of the forward and the backward chain's masks at the gap's frames first..first + n - 1; `span` the distance between the two
    keys.  fp32 [n, H, W].  One launch."""
    int_in(span, 2, 65535, "span")
    int_in(first, 1, span - 1, "first")
    require_hip(qa, "qa", __name__)
    require_hip(qb, "qb", __name__)
    if qa.ndim != 3 or not 1 <= qa.shape[0] <= span - first:
        raise ValueError(f"qa must be [n, H, W] with first + n - 1 <= span - 1, got {tuple(qa.shape)}")
    tensor_is(qa, torch.int32, qa.shape, "qa", __name__)
    tensor_is(qb, torch.int32, qa.shape, "qb", __name__)
    n, H, W = qa.shape
    check_plane(H, W)
    out = torch.empty((n, H, W), dtype=torch.float32, device=qa.device) if out is None else out
    d = _cabi.LpPropMergeDesc(n, H, W, span, first, 0, qa.data_ptr(), qb.data_ptr(), out.data_ptr())
    launch("lp_prop_merge", qa.device, ctypes.byref(d))
    return out


def clip_pyramids(images, levels):
    """The luma pyramids of all frames, uint8 [F, stride], held whole under WS_CAP_BYTES; input that needs a conversion to
    contiguous fp32 goes through it in chunks of frames under WS_CAP_BYTES."""
    F, H, W, _ = images.shape
    stride = _cabi.prop_pyramid_ws_bytes(1, H, W, levels)
    if F * stride > WS_CAP_BYTES:
        raise ValueError(f"the luma pyramids of {F} frames of {H}x{W} take {F * stride} bytes, above WS_CAP_BYTES = {WS_CAP_BYTES}")
    return luma_pyramids(images, levels, torch.empty((F, stride), dtype=torch.uint8, device=images.device), WS_CAP_BYTES)


class Chains:
    """What outlives a step of the chains of a call -- per chain two position maps and two mask pyramids, and the addresses of
    its key, its frames' luma and its outputs -- and the advance's job table.  The fields are scratch within a step: they are
    the rows of a `FieldWalk`, which belong to the j-th chain of the group being launched.  A table is a host uint64 array of
    device addresses; step s of chain c reads and writes at addresses that are linear in s or alternate with its parity, so a
    step fills columns with a few numpy operations and allocates nothing on the device."""

    def __init__(self, plan, pyr, key_pyrs, outs, H, W, levels, search, smooth):
        dev = pyr.device
        self.dev = dev
        self.length = np.array([c[3] for c in plan], dtype=np.int64)
        stride = pyr.shape[1]
        self.walk = FieldWalk(min(len(plan), MAX_JOBS), H, W, levels, search, smooth, dev)
        self._keep = []                                              # the device buffers behind the addresses
        self.pos = [self._buffers((H, W, 2), torch.int32) for _ in range(2)]
        self.mpyr = [self._buffers((stride,), torch.uint8) for _ in range(2)]
        self.key = np.array([key_pyrs[c[0]].data_ptr() for c in plan], dtype=np.uint64)
        # frame k + d s of the clip's pyramids, and where step s writes its mask: both base + s * step, the step signed
        self.luma0 = np.array([pyr.data_ptr() + c[1] * stride for c in plan], dtype=np.int64)
        self.luma_step = np.array([c[2] * stride for c in plan], dtype=np.int64)
        self.out0 = np.array([o[0] for o in outs], dtype=np.int64)
        self.out_step = np.array([o[1] for o in outs], dtype=np.int64)
        self.t_advance = np.zeros((len(self.walk.field0), 6), dtype=np.uint64)
        self.t_advance[:, 0] = self.walk.field0
        self.advance_desc = _cabi.LpPropAdvanceBatchDesc(H, W, levels, 0, self.t_advance.ctypes.data)

    def _buffers(self, shape, dtype):
        """One buffer of `shape` per chain: their addresses."""
        self._keep.append(torch.empty((len(self.length), *shape), dtype=dtype, device=self.dev))
        return row_addresses(self._keep[-1], len(self.length))

    def step(self, s):
        """Step s of every chain that has one: 2 levels + 1 launches per MAX_JOBS chains."""
        idx = np.flatnonzero(self.length >= s)
        for lo in range(0, len(idx), MAX_JOBS):
            self._bind(s, idx[lo:lo + MAX_JOBS])
            self._launch(min(MAX_JOBS, len(idx) - lo))

    def _bind(self, s, idx):
        """The tables' rows 0 .. len(idx) - 1 for step s of the chains `idx`, one group."""
        n = len(idx)
        self.luma = (self.luma0[idx] + s * self.luma_step[idx]).astype(np.uint64)        # the frame the step arrives at
        self.jobs = ((self.luma0[idx] + (s - 1) * self.luma_step[idx]).astype(np.uint64), self.luma,
                     self.key[idx] if s == 1 else self.mpyr[(s - 1) & 1][idx])
        a = self.t_advance
        a[:n, 1] = 0 if s == 1 else self.pos[(s - 1) & 1][idx]
        a[:n, 2], a[:n, 3], a[:n, 5] = self.key[idx], self.pos[s & 1][idx], self.mpyr[s & 1][idx]
        a[:n, 4] = (self.out0[idx] + s * self.out_step[idx]).astype(np.uint64)

    def _launch(self, n):
        """The launches of the group of `n` chains that was bound."""
        self.walk.run(*self.jobs)
        self.advance_desc.jobs = n
        launch("lp_prop_advance_batch", self.dev, ctypes.byref(self.advance_desc))


def _key_masks(masks, keys, F, H, W):
    """The K key masks as a list of [H, W] tensors."""
    if masks.ndim == 2 and len(keys) == 1:
        masks = masks.unsqueeze(0)
    if masks.ndim != 3 or masks.shape[0] not in (len(keys), F) or tuple(masks.shape[1:]) != (H, W):
        raise ValueError(f"masks {tuple(masks.shape)} do not match {len(keys)} keys in {F} frames of {H}x{W}: [K, H, W], "
                         "[F, H, W], or [H, W] for one key")
    return [masks[i] for i in (range(len(keys)) if masks.shape[0] == len(keys) else keys)]


def painted_keys(images, masks, key_frames, levels, module, planes=1):
    """What the two several-keys forms start from: (the plan, the keys, the pyramid of every key's bits, `planes` outputs fp32
    [F, H, W]: on the key frames the first holds the binarised paintings and the others zero).  `module` is the caller's
    __name__.  One launch per key."""
    if not torch.is_tensor(images) or images.ndim != 4:
        check_images(images)                                         # raises: the frame count is needed for the keys' check
    plan = chain_plan(images.shape[0], key_frames)                   # the numbers before the tensors
    keys = list(key_frames)
    check_images(images)
    require_hip(masks, "masks", module)
    (F, H, W, _), dev = images.shape, images.device
    outs = [torch.empty((F, H, W), dtype=torch.float32, device=dev) for _ in range(planes)]
    key_pyrs = []
    for k, m in zip(keys, _key_masks(masks, keys, F, H, W)):
        mpyr, bits = key_mask(m.to(dev), levels)
        key_pyrs.append(mpyr)
        outs[0][k] = bits
        for o in outs[1:]:
            o[k].zero_()
    return plan, keys, key_pyrs, outs


def propagate_keys(images, masks, key_frames, levels=4, search=2, smooth=8):
    """The masks painted on the frames `key_frames` of `images` [F, H, W, C], followed through every frame and merged between
    the keys (module docstring): fp32 [F, H, W] on the images' device.  No device -> host read."""
    check_params(levels, search, smooth)
    plan, keys, key_pyrs, (out,) = painted_keys(images, masks, key_frames, levels, __name__)
    (F, H, W, _), dev = images.shape, images.device
    if not plan:
        return out
    # a gap's forward chain writes into `out`, its backward chain into `back`; the merge then overwrites the gap's frames of `out`
    gaps = [(a, b) for a, b in zip(keys, keys[1:]) if b - a > 1]
    back = torch.empty((sum(b - a - 1 for a, b in gaps), H, W), dtype=torch.float32, device=dev)
    back_at, n = {}, 0
    for a, b in gaps:
        back_at[b] = back[n:n + b - a - 1]
        n += b - a - 1
    plane = H * W * 4
    outs = []
    for i, k, d, length in plan:
        if d < 0 and i > 0:                                          # frame k - s is row (k - s) - (k - length) of the gap's stack
            outs.append((back_at[k].data_ptr() + length * plane, -plane))
        else:
            outs.append((out.data_ptr() + k * plane, d * plane))
    pyr = clip_pyramids(images, levels)
    chains = Chains(plan, pyr, key_pyrs, outs, H, W, levels, search, smooth)
    for s in range(1, int(chains.length.max()) + 1):
        chains.step(s)
    for a, b in gaps:
        mid = out[a + 1:b]
        merge_gap(stabilize.signed_d2(mid), stabilize.signed_d2(back_at[b]), b - a, 1, mid)
    return out
