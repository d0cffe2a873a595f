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
        second key is what recovers it); what leaves the picture.  Lost chains are not stopped early.  On a long clip whose
        subject moves a fraction of a pixel per frame drift reads as occlusion here: propagate_keys_anchored_visible.py anchors
        every chain of this form, and shares this module's chains and merge (`visible_chains`).

HIP tensors only, no CPU fallback, no device -> host read: the visible bits are counted by the occlude launch (an integer atomic
add per chain and step) and the lost decision is taken inside the merge launch.  A step is 2 levels + 3 launches per 32 active
chains and allocates nothing.  The forward chain of a gap keeps its code and its mask in the call's own outputs (`hidden` holds the
code until the merge, which works in place); the backward chain's code and mask and both chains' flags are kept per in-between
frame, for all gaps at once, and must fit WS_CAP_BYTES; the distances and the merge go in chunks of frames under WS_CAP_BYTES.
"""
from __future__ import annotations

import ctypes

import torch

from . import _cabi, propagate_keys, stabilize
from ._hostcall import chunks, int_in, launch, require_hip, tensor_is
from ._motion import MAX_JOBS, check_frame_planes, check_params, check_plane              # noqa: F401  (MAX_JOBS: this module's to export)
from .propagate_keys import Chains, Gaps, chain_plan, clip_pyramids, job_table, painted_keys     # noqa: F401  (chain_plan: the node's)
from .propagate_visible import DEFAULT_OCCLUSION, MAX_OCCLUSION, check_occlude

WS_CAP_BYTES = 1 << 30


def visible_flags_batch(jobs, occlusion=DEFAULT_OCCLUSION):
    """`propagate_visible.visible_flags` for several independent steps of one plane in one launch.  `jobs`: per job (pos, tgt, key,
    mask_bits) as there.  A list of flags int32 [gh, gw]."""
    int_in(occlusion, 1, MAX_OCCLUSION, "occlusion")
    plane = (None, None)
    for job in jobs:
        H, W = plane = check_frame_planes(*job, __name__, plane)    # the first job's plane is every job's
    rows = [(*job, torch.empty(_cabi.prop_grid(H, W), dtype=torch.int32, device=job[1].device)) for job in jobs]
    table = job_table(rows, "visible_flags_batch")
    d = _cabi.LpPropVisibleBatchDesc(H, W, occlusion, len(rows), table.ctypes.data)
    launch("lp_prop_visible_batch", rows[0][1].device, ctypes.byref(d))
    return [r[4] for r in rows]


def occlude_batch(jobs, levels, counts=None):
    """`propagate_visible.occlude` for several independent steps of one plane in one launch.  `jobs`: per job (code, flags).
    `counts`, an int32 [jobs] tensor, receives += the number of visible bits per job.  A list of (mask, hidden, the pyramid of
    the visible bits)."""
    int_in(levels, 1, _cabi.LP_PROP_MAX_LEVELS, "levels")            # the number before `counts`, a tensor, is looked at
    if counts is not None:
        tensor_is(counts, torch.int32, (len(jobs),), "counts", __name__)
    plane = (None, None)
    for job in jobs:
        H, W = plane = check_occlude(*job, levels, __name__, plane)

    def new(dev):
        return (torch.empty((H, W), dtype=torch.float32, device=dev), torch.empty((H, W), dtype=torch.float32, device=dev),
                torch.empty((1, _cabi.prop_pyramid_ws_bytes(1, H, W, levels)), dtype=torch.uint8, device=dev))
    rows = [(*job, *new(job[0].device), None if counts is None else counts[i:]) for i, job in enumerate(jobs)]
    table = job_table(rows, "occlude_batch")
    d = _cabi.LpPropOccludeBatchDesc(H, W, levels, len(rows), table.ctypes.data)
    launch("lp_prop_occlude_batch", rows[0][0].device, ctypes.byref(d))
    return [r[2:5] for r in rows]


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


def propagate_keys_visible(images, masks, key_frames, levels=4, search=2, smooth=8, occlusion=DEFAULT_OCCLUSION):
    """The masks painted on the frames `key_frames` of `images` [F, H, W, C], followed through every frame, kept off what passes
    in front and merged between the keys (module docstring): (mask, hidden), fp32 [F, H, W] each, on the images' device.  No
    device -> host read."""
    check_params(levels, search, smooth)
    int_in(occlusion, 0, MAX_OCCLUSION, "occlusion")
    if occlusion == 0:                                               # the plain form makes every further check itself
        out = propagate_keys.propagate_keys(images, masks, key_frames, levels, search, smooth)
        return out, torch.zeros_like(out)
    return visible_chains(images, masks, key_frames, levels, search, smooth, occlusion, __name__, WS_CAP_BYTES)


def visible_chains(images, masks, key_frames, levels, search, smooth, occlusion, module, cap, anchor=0):
    """The occlusion-aware chains of a call and their merge, the numbers checked: what propagate_keys_visible is behind its "off"
    route.  `module` and `cap` are the caller's __name__ and WS_CAP_BYTES.  `anchor` above 0 makes every chain the anchored
    occlusion-aware chain of its key (propagate_keys_anchored_visible.py): the chain table's second option next to the first,
    and a position map per chain more to keep."""
    plan, keys, key_pyrs, (out, hidden) = painted_keys(images, masks, key_frames, levels, module, 2)
    (F, H, W, _), dev = images.shape, images.device
    if not plan:
        return out, hidden
    gaps = Gaps(keys)
    between = gaps.between
    gh, gw = _cabi.prop_grid(H, W)
    plane, cells = H * W * 4, gh * gw * 4
    kept = between * 2 * (plane + cells) + (len(plan) + 1) * (plane + cells) + (len(plan) * 2 * plane if anchor else 0)
    if kept > cap:
        more = f" and the position maps of {len(plan)} anchored chains" if anchor else ""
        raise ValueError(f"the backward chains' codes and masks and the flags of {between} in-between frames of {H}x{W}{more} take "
                         f"{kept} bytes, above WS_CAP_BYTES = {cap}: paint fewer frames apart or split the clip")
    back = torch.empty((2, between, H, W), dtype=torch.float32, device=dev)              # the backward chains' code and mask
    flags = torch.empty((2, between, gh, gw), dtype=torch.int32, device=dev)            # the forward and the backward chains'
    scratch = torch.empty((len(plan), H, W), dtype=torch.float32, device=dev)           # an edge chain's code, a gap chain's hidden
    scratch_flags = torch.empty((len(plan) + 1, gh, gw), dtype=torch.int32, device=dev)   # an edge chain's flags; the last: no flag
    counts = torch.zeros(2 * sum(b - a for a, b in gaps.pairs), dtype=torch.int32, device=dev)   # per gap [span] forward, [span] backward
    # a gap's counts lie behind those of the g gaps before it, which take 2 (b - a) = 2 (b - a - 1) + 2 each
    count_of = {gap: 2 * (gaps.first[gap] + g) for g, gap in enumerate(gaps.pairs)}
    code, mask, hid, flag, count = [], [], [], [], []
    for c, chain in enumerate(plan):
        gap, forward = gaps.of(chain), chain[2] > 0
        tmp = gaps.fixed(scratch, c)
        if gap is None:                                              # outside the keys: the chain's own outputs, no count
            code.append(tmp)
            mask.append(gaps.in_place(out, chain))
            hid.append(gaps.in_place(hidden, chain))
            flag.append(gaps.fixed(scratch_flags, c))
            count.append((0, 0))
        else:                                # a gap's forward chain in place in the outputs, its backward chain in the stacks
            code.append(gaps.in_place(hidden, chain) if forward else gaps.stacked(back[0], chain))
            mask.append(gaps.in_place(out, chain) if forward else gaps.stacked(back[1], chain))
            hid.append(tmp)
            flag.append(gaps.stacked(flags[0 if forward else 1], chain))
            count.append((counts[count_of[gap] + (0 if forward else gap[1] - gap[0]):].data_ptr(), 4))
    pyr = clip_pyramids(images, levels)
    chains = Chains(plan, pyr, key_pyrs, code, H, W, levels, search, smooth, split=(occlusion, mask, hid, flag, count),
                    rematch=(anchor, occlusion) if anchor else None)
    if gaps.pairs:
        scratch_flags[-1].zero_()
        chains.count_keys([out[k] for _, k, _, _ in plan], scratch_flags[-1])
    for s in range(1, int(chains.length.max()) + 1):
        chains.step(s)
    for a, b in gaps.pairs:
        r, span = gaps.first[a, b], b - a
        count_a, count_b = counts[count_of[a, b]:][:span], counts[count_of[a, b] + span:][:span]
        for s, n in chunks(span - 1, 2 * plane, cap):                # the two chains' distances of a chunk's frames
            code_a, mask_a = hidden[a + 1 + s:a + 1 + s + n], out[a + 1 + s:a + 1 + s + n]
            code_b, mask_b = back[0, r + s:r + s + n], back[1, r + s:r + s + n]
            merge_gap_visible(stabilize.signed_d2(code_a), stabilize.signed_d2(code_b), code_a, mask_a, code_b, mask_b,
                              flags[0, r + s:r + s + n], flags[1, r + s:r + s + n], count_a, count_b, span, 1 + s, mask_a, code_a)
    return out, hidden
