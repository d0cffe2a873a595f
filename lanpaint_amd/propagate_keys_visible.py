"""Video mask propagate from several keyframes, occlusion-aware: every painted key follows the picture's motion in both directions
and stays off what passes in front of the subject, and between two keys a chain that lost the subject gives way to the other.

`propagate_keys.propagate_keys` honours several painted keys and has no occlusion handling; `propagate_visible` keeps the mask off
an occluder but has one key, and a subject that is hidden entirely is lost.  The remedy a user reaches for is a second key painted
behind the occluder.  This joins the two:

propagate_keys_visible(images, masks, key_frames, levels=4, search=2, smooth=8, occlusion=16) -> (mask [F, H, W], hidden [F, H, W])
        `images`, `masks` and `key_frames` as in `propagate_keys`, `occlusion` as in `propagate_masks_visible`.  Every chain of
        `chain_plan` is the occlusion-aware chain started from its own key and tested against that key's picture.  A key frame
        returns its binarised painted mask and a zero `hidden`; a frame in front of the first or behind the last key its one
        chain's (mask, hidden).  Between two keys a and b: a chain is lost once fewer than 16 of its pixels were visible in some
        frame on its way (its key had at least 16), and stays lost.  With exactly one chain lost the frame is the other chain's,
        bit for bit.  Otherwise the subjects (mask + hidden of either chain) are merged through their signed distances as
        `propagate_keys` merges, the merged value is rounded to a code of 1/256, and the block flags of the chain from the nearer
        key split it into `mask` and `hidden`.  One key gives `propagate_masks_visible` bit for bit; occlusion = 0 gives
        `propagate_keys` and zeros with no further launch; a still video with the same mask on every key returns that binarised
        mask and a zero `hidden`; empty keys everywhere give 0 and 0; mask + hidden is a multiple of 1/256.  include/lanpaint_hip.h
        (lp_prop_visible_batch, lp_prop_occlude_batch, lp_prop_merge_visible) states the rule in full.  Not handled: occlusion
        edges finer than a block; following a subject through a full occlusion (positions stall while nothing is visible: the
        second key is what recovers it); what leaves the picture.  Lost chains are not stopped early.

HIP tensors only, no CPU fallback, no device -> host read: the visible bits are counted by the occlude launch (an integer atomic
add per chain and step) and the lost decision is taken inside the merge launch.  A step is 2 levels + 3 launches per 32 active
chains and allocates nothing.  The forward chain of a gap keeps its code and its mask in the call's own outputs (`hidden` holds the
code until the merge, which works in place); the backward chain's code and mask and both chains' flags are kept per in-between
frame, for all gaps at once, and must fit WS_CAP_BYTES; the distances and the merge go in chunks of frames under WS_CAP_BYTES.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _cabi, propagate_keys, stabilize
from ._hostcall import chunks, int_in, launch, require_hip, tensor_is
from ._motion import MAX_JOBS, check_params, check_plane
from .propagate_keys import Chains, chain_plan, clip_pyramids, job_table, painted_keys     # noqa: F401  (chain_plan: the node's)
from .propagate_visible import DEFAULT_OCCLUSION, MAX_OCCLUSION

WS_CAP_BYTES = 1 << 30


def visible_flags_batch(jobs, occlusion=DEFAULT_OCCLUSION):
    """`propagate_visible.visible_flags` for several independent steps of one plane in one launch.  `jobs`: per job (pos, tgt, key,
    mask_bits) as there.  A list of flags int32 [gh, gw]."""
    int_in(occlusion, 1, MAX_OCCLUSION, "occlusion")
    rows = []
    for pos, tgt, key, mask_bits in jobs:
        H, W = tensor_is(tgt, torch.uint8, rows[0][1].shape if rows else (None, None), "tgt", __name__).shape
        check_plane(H, W)
        tensor_is(key, torch.uint8, (H, W), "key", __name__)
        tensor_is(mask_bits, torch.uint8, (H, W), "mask_bits", __name__)
        tensor_is(pos, torch.int32, (H, W, 2), "pos", __name__)
        rows.append((pos, tgt, key, mask_bits, torch.empty(_cabi.prop_grid(H, W), dtype=torch.int32, device=tgt.device)))
    table = job_table(rows, "visible_flags_batch")
    H, W = rows[0][1].shape
    d = _cabi.LpPropVisibleBatchDesc(H, W, occlusion, len(rows), table.ctypes.data)
    launch("lp_prop_visible_batch", rows[0][1].device, ctypes.byref(d))
    return [r[4] for r in rows]


def occlude_batch(jobs, levels, counts=None):
    """`propagate_visible.occlude` for several independent steps of one plane in one launch.  `jobs`: per job (code, flags).
    `counts`, an int32 [jobs] tensor, receives += the number of visible bits per job.  A list of (mask, hidden, the pyramid of
    the visible bits)."""
    int_in(levels, 1, _cabi.LP_PROP_MAX_LEVELS, "levels")
    rows, outs = [], []
    if counts is not None:
        tensor_is(counts, torch.int32, (len(jobs),), "counts", __name__)
    for i, (code, flags) in enumerate(jobs):
        H, W = tensor_is(code, torch.float32, rows[0][0].shape if rows else (None, None), "code", __name__).shape
        check_plane(H, W)
        tensor_is(flags, torch.int32, _cabi.prop_grid(H, W), "flags", __name__)
        dev = code.device
        new = (torch.empty((H, W), dtype=torch.float32, device=dev), torch.empty((H, W), dtype=torch.float32, device=dev),
               torch.empty((1, _cabi.prop_pyramid_ws_bytes(1, H, W, levels)), dtype=torch.uint8, device=dev))
        rows.append((code, flags, *new, None if counts is None else counts[i:]))
        outs.append(new)
    table = job_table(rows, "occlude_batch")
    H, W = rows[0][0].shape
    d = _cabi.LpPropOccludeBatchDesc(H, W, levels, len(rows), table.ctypes.data)
    launch("lp_prop_occlude_batch", rows[0][0].device, ctypes.byref(d))
    return outs


def merge_gap_visible(qa, qb, code_a, mask_a, code_b, mask_b, flags_a, flags_b, count_a, count_b, span, first=1, out=None, hidden=None):
    """The merge of one gap's in-between frames first..first + n - 1: `qa`, `qb` int32 [n, H, W], the signed squared distances of
    the two chains' subject bits; their codes and masks fp32 [n, H, W]; their flags int32 [n, gh, gw]; their visible-bit counts
    int32 [span] by step.  (mask, hidden) fp32 [n, H, W]; `out` may be `mask_a` and `hidden` may be `code_a`.  One launch."""
    int_in(span, 2, 65535, "span")
    int_in(first, 1, span - 1, "first")
    require_hip(qa, "qa", __name__)
    if qa.ndim != 3 or not 1 <= qa.shape[0] <= span - first:
        raise ValueError(f"qa must be [n, H, W] with first + n - 1 <= span - 1, got {tuple(qa.shape)}")
    n, H, W = qa.shape
    check_plane(H, W)
    i32, f32, grid = torch.int32, torch.float32, _cabi.prop_grid(H, W)
    for t, dtype, shape, what in ((qa, i32, (n, H, W), "qa"), (qb, i32, (n, H, W), "qb"), (code_a, f32, (n, H, W), "code_a"),
                                  (mask_a, f32, (n, H, W), "mask_a"), (code_b, f32, (n, H, W), "code_b"),
                                  (mask_b, f32, (n, H, W), "mask_b"), (flags_a, i32, (n, *grid), "flags_a"),
                                  (flags_b, i32, (n, *grid), "flags_b"), (count_a, i32, (span,), "count_a"),
                                  (count_b, i32, (span,), "count_b")):
        tensor_is(t, dtype, shape, what, __name__)
    out = torch.empty((n, H, W), dtype=torch.float32, device=qa.device) if out is None else out
    hidden = torch.empty((n, H, W), dtype=torch.float32, device=qa.device) if hidden is None else hidden
    d = _cabi.LpPropMergeVisibleDesc(n, H, W, span, first, 0, qa.data_ptr(), qb.data_ptr(), code_a.data_ptr(), mask_a.data_ptr(),
                                     code_b.data_ptr(), mask_b.data_ptr(), flags_a.data_ptr(), flags_b.data_ptr(),
                                     count_a.data_ptr(), count_b.data_ptr(), out.data_ptr(), hidden.data_ptr())
    launch("lp_prop_merge_visible", qa.device, ctypes.byref(d))
    return out, hidden


class VisibleChains(Chains):
    """`propagate_keys.Chains` with the two launches of the occlusion-aware form behind every advance.  The advance's code goes
    where `code` says (the base class's `outs`) and its pyramid to a buffer per chain; `mask`, `hidden`, `flags` and `count` say,
    as (address, step in bytes) per chain, where step s writes the visible part, the hidden part, the flags and the number of
    visible bits (address 0: not counted).  The key frame's luma is level 0 of its pyramid in `pyr`."""

    def __init__(self, plan, pyr, key_pyrs, code, mask, hidden, flags, count, H, W, levels, search, smooth, occlusion):
        super().__init__(plan, pyr, key_pyrs, code, H, W, levels, search, smooth)
        self.raw_mpyr = self._buffers((pyr.shape[1],), torch.uint8)
        self.lin = [(np.array([o[0] for o in col], dtype=np.int64), np.array([o[1] for o in col], dtype=np.int64))
                    for col in (mask, hidden, flags, count)]
        self.t_visible = np.zeros((len(self.t_advance), 5), dtype=np.uint64)
        self.t_occlude = np.zeros((len(self.t_advance), 6), dtype=np.uint64)
        self.visible_desc = _cabi.LpPropVisibleBatchDesc(H, W, occlusion, 0, self.t_visible.ctypes.data)
        self.occlude_desc = _cabi.LpPropOccludeBatchDesc(H, W, levels, 0, self.t_occlude.ctypes.data)

    def _bind(self, s, idx):
        super()._bind(s, idx)
        n = len(idx)
        a, v, o = self.t_advance, self.t_visible, self.t_occlude
        a[:n, 5] = self.raw_mpyr[idx]
        at = [(base[idx] + s * step[idx]).astype(np.uint64) for base, step in self.lin]
        v[:n, 0], v[:n, 1], v[:n, 2], v[:n, 3], v[:n, 4] = a[:n, 3], self.luma, self.luma0[idx].astype(np.uint64), a[:n, 5], at[2]
        o[:n, 0], o[:n, 1], o[:n, 2], o[:n, 3], o[:n, 4], o[:n, 5] = a[:n, 4], at[2], at[0], at[1], self.mpyr[s & 1][idx], at[3]

    def _launch(self, n):
        super()._launch(n)
        self.visible_desc.jobs = self.occlude_desc.jobs = n
        launch("lp_prop_visible_batch", self.dev, ctypes.byref(self.visible_desc))
        launch("lp_prop_occlude_batch", self.dev, ctypes.byref(self.occlude_desc))

    def count_keys(self, painted, zero_flags):
        """Entry 0 of every counted chain's counts: the key's bits, counted by the occlude launch on the key's binarised mask with
        no block flagged.  `painted`: per chain the key's fp32 bits.  What it writes besides goes to buffers that step 1 or 2
        overwrites before they are read: the chain's hidden scratch, a position map and a pyramid."""
        rows = [(painted[c].data_ptr(), zero_flags.data_ptr(), int(self.pos[0][c]), int(self.lin[1][0][c]), int(self.mpyr[0][c]),
                 int(self.lin[3][0][c])) for c in range(len(self.length)) if self.lin[3][0][c]]
        table = np.array(rows, dtype=np.uint64).reshape(len(rows), 6)
        for lo in range(0, len(rows), MAX_JOBS):                         # through the occlude table, a group at a time
            n = self.occlude_desc.jobs = min(MAX_JOBS, len(rows) - lo)
            self.t_occlude[:n] = table[lo:lo + n]
            launch("lp_prop_occlude_batch", self.dev, ctypes.byref(self.occlude_desc))


def propagate_keys_visible(images, masks, key_frames, levels=4, search=2, smooth=8, occlusion=DEFAULT_OCCLUSION):
    """The masks painted on the frames `key_frames` of `images` [F, H, W, C], followed through every frame, kept off what passes
    in front and merged between the keys (module docstring): (mask, hidden), fp32 [F, H, W] each, on the images' device.  No
    device -> host read."""
    check_params(levels, search, smooth)
    int_in(occlusion, 0, MAX_OCCLUSION, "occlusion")
    if occlusion == 0:                                               # the plain form makes every further check itself
        out = propagate_keys.propagate_keys(images, masks, key_frames, levels, search, smooth)
        return out, torch.zeros_like(out)
    plan, keys, key_pyrs, (out, hidden) = painted_keys(images, masks, key_frames, levels, __name__, 2)
    (F, H, W, _), dev = images.shape, images.device
    if not plan:
        return out, hidden
    gaps = [(a, b) for a, b in zip(keys, keys[1:]) if b - a > 1]
    between = sum(b - a - 1 for a, b in gaps)
    gh, gw = _cabi.prop_grid(H, W)
    plane, cells = H * W * 4, gh * gw * 4
    kept = between * 2 * (plane + cells) + (len(plan) + 1) * (plane + cells)
    if kept > WS_CAP_BYTES:
        raise ValueError(f"the backward chains' codes and masks and the flags of {between} in-between frames of {H}x{W} take {kept} "
                         f"bytes, above WS_CAP_BYTES = {WS_CAP_BYTES}: paint fewer frames apart or split the clip")
    back = torch.empty((2, between, H, W), dtype=torch.float32, device=dev)              # the backward chains' code and mask
    flags = torch.empty((2, between, gh, gw), dtype=torch.int32, device=dev)            # the forward and the backward chains'
    scratch = torch.empty((len(plan), H, W), dtype=torch.float32, device=dev)           # an edge chain's code, a gap chain's hidden
    scratch_flags = torch.empty((len(plan) + 1, gh, gw), dtype=torch.int32, device=dev)   # an edge chain's flags; the last: no flag
    counts = torch.zeros(2 * sum(b - a for a, b in gaps), dtype=torch.int32, device=dev)     # per gap [span] forward, [span] backward
    row_of, count_of, n, m = {}, {}, 0, 0
    for a, b in gaps:
        row_of[a, b], count_of[a, b] = n, m
        n, m = n + b - a - 1, m + 2 * (b - a)
    code, mask, hid, flag, count = [], [], [], [], []
    for c, (i, k, d, length) in enumerate(plan):
        tmp, tmp_flags = (scratch[c].data_ptr(), 0), (scratch_flags[c].data_ptr(), 0)
        if d > 0 and i < len(keys) - 1:                              # a gap's forward chain: frame k + s, in place in the outputs
            gap = (k, keys[i + 1])
            code.append((hidden.data_ptr() + k * plane, plane))
            mask.append((out.data_ptr() + k * plane, plane))
            hid.append(tmp)
            flag.append((flags[0, row_of[gap]].data_ptr() - cells, cells))
            count.append((counts[count_of[gap]:].data_ptr(), 4))
        elif d < 0 and i > 0:                                        # a gap's backward chain: frame k - s is row length - s of its stack
            gap = (keys[i - 1], k)
            code.append((back[0, row_of[gap]].data_ptr() + length * plane, -plane))
            mask.append((back[1, row_of[gap]].data_ptr() + length * plane, -plane))
            hid.append(tmp)
            flag.append((flags[1, row_of[gap]].data_ptr() + length * cells, -cells))
            count.append((counts[count_of[gap] + (k - gap[0]):].data_ptr(), 4))
        else:                                                        # outside the keys: the chain's own output
            code.append(tmp)
            mask.append((out.data_ptr() + k * plane, d * plane))
            hid.append((hidden.data_ptr() + k * plane, d * plane))
            flag.append(tmp_flags)
            count.append((0, 0))
    pyr = clip_pyramids(images, levels)
    chains = VisibleChains(plan, pyr, key_pyrs, code, mask, hid, flag, count, H, W, levels, search, smooth, occlusion)
    if gaps:
        scratch_flags[-1].zero_()
        chains.count_keys([out[k] for _, k, _, _ in plan], scratch_flags[-1])
    for s in range(1, int(chains.length.max()) + 1):
        chains.step(s)
    for a, b in gaps:
        r, span = row_of[a, b], b - a
        count_a, count_b = counts[count_of[a, b]:][:span], counts[count_of[a, b] + span:][:span]
        for s, n in chunks(span - 1, 2 * plane, WS_CAP_BYTES):       # the two chains' distances of a chunk's frames
            code_a, mask_a = hidden[a + 1 + s:a + 1 + s + n], out[a + 1 + s:a + 1 + s + n]
            code_b, mask_b = back[0, r + s:r + s + n], back[1, r + s:r + s + n]
            merge_gap_visible(stabilize.signed_d2(code_a), stabilize.signed_d2(code_b), code_a, mask_a, code_b, mask_b,
                              flags[0, r + s:r + s + n], flags[1, r + s:r + s + n], count_a, count_b, span, 1 + s, mask_a, code_a)
    return out, hidden
