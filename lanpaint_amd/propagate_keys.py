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
from ._motion import MAX_JOBS, MAX_SEARCH, FieldWalk, check_images, check_params, check_plane, luma_pyramids, row_addresses
from .propagate import check_advance, check_field, check_match, key_mask

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
    for job in jobs:
        gh, gw = check_match(*job, H, W, levels, level, search, smooth, __name__)
    rows = [(*job, torch.empty((gh, gw, 2), dtype=torch.int32, device=job[0].device),
             torch.empty((gh, gw), dtype=torch.int32, device=job[0].device)) for job in jobs]
    table = job_table(rows, "match_level_batch")
    d = _cabi.LpPropMatchBatchDesc(H, W, levels, level, search, smooth, len(rows), 0, table.ctypes.data)
    launch("lp_prop_match_batch", rows[0][0].device, ctypes.byref(d))
    return [r[4:] for r in rows]


def anchor_field_batch(jobs, H, W, levels, anchor=2, smooth=8, occlusion=0):
    """`propagate_anchored.anchor_field` for several independent frames in one launch: lp_prop_match_batch in its warped-key form.
    `jobs`: per job (key, tgt, mpyr, pos): the key frame's and the frame's luma pyramid, the pyramid of the bits the advance wrote
    and the frame's positions int32 [H, W, 2].  A list of (vec int32 [gh, gw, 2], valid int32 [gh, gw]), what fill_median takes.
    `occlusion` above 0, up to 255, selects the gated form: `propagate_anchored_visible.gated_anchor_field`'s vec and valid per
    job, with no `gated` plane."""
    int_in(anchor, 1, MAX_SEARCH, "anchor")
    int_in(occlusion, 0, 255, "occlusion")
    check_params(levels, anchor, smooth)
    for key, tgt, mpyr, pos in jobs:
        check_match(key, tgt, mpyr, None, H, W, levels, levels - 1, anchor, smooth, __name__)    # the numbers and three pyramids
        tensor_is(pos, torch.int32, (H, W, 2), "pos", __name__)
    gh, gw = _cabi.prop_grid(H, W)
    rows = [(*job, torch.empty((gh, gw, 2), dtype=torch.int32, device=job[0].device),
             torch.empty((gh, gw), dtype=torch.int32, device=job[0].device)) for job in jobs]
    table = job_table(rows, "anchor_field_batch")
    form = _cabi.LP_PROP_MATCH_GATED(occlusion) if occlusion else _cabi.LP_PROP_MATCH_WARPED_KEY
    d = _cabi.LpPropMatchBatchDesc(H, W, levels, 0, anchor, smooth, len(rows), form, table.ctypes.data)
    launch("lp_prop_match_batch", rows[0][0].device, ctypes.byref(d))
    return [r[4:] for r in rows]


def fill_median_batch(jobs):
    """`propagate.fill_median` for several fields of one grid in one launch.  `jobs`: per job (vec, valid).  A list of fields."""
    grid = (None, None)
    for vec, valid in jobs:
        gh, gw = grid = check_field(vec, valid, __name__, grid)     # the first job's grid is every job's
    rows = [(vec, valid, torch.empty_like(vec)) for vec, valid in jobs]
    table = job_table(rows, "fill_median_batch")
    launch("lp_prop_fill_batch", rows[0][0].device, table.ctypes.data, len(rows), gh, gw)
    return [r[2] for r in rows]


def advance_batch(jobs, levels):
    """`propagate.advance` for several independent steps of one plane in one launch.  `jobs`: per job (vec, pos, key_bits), `pos`
    None for the key frame's positions.  A list of (positions, mask fp32 [H, W], the pyramid of its bits uint8 [1, stride])."""
    plane = (None, None)
    for job in jobs:
        H, W = plane = check_advance(*job, levels, __name__, plane)  # the first job's plane is every job's

    def new(dev):
        return (torch.empty((H, W, 2), dtype=torch.int32, device=dev), torch.empty((H, W), dtype=torch.float32, device=dev),
                torch.empty((1, _cabi.prop_pyramid_ws_bytes(1, H, W, levels)), dtype=torch.uint8, device=dev))
    rows = [(*job, *new(job[0].device)) for job in jobs]
    table = job_table(rows, "advance_batch")
    d = _cabi.LpPropAdvanceBatchDesc(H, W, levels, len(rows), table.ctypes.data)
    launch("lp_prop_advance_batch", rows[0][0].device, ctypes.byref(d))
    return [r[3:] for r in rows]


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


class Gaps:
    """Where the chains of a call write.  `pairs`: the key pairs (a, b) that have frames between them; `first[a, b]`: the gap's
    first row in a stack of all in-between frames, gap after gap; `between`: their number.  The other methods say where step s of
    a chain of `chain_plan` goes in a contiguous tensor, as (address, byte step): address + s * step, the step signed."""

    def __init__(self, keys):
        self.keys = keys
        self.pairs = [(a, b) for a, b in zip(keys, keys[1:]) if b - a > 1]
        self.first, self.between = {}, 0
        for a, b in self.pairs:
            self.first[a, b] = self.between
            self.between += b - a - 1

    def of(self, chain):
        """The gap a chain runs in; None for an edge chain, in front of the first or behind the last key."""
        i, k, d, _ = chain
        if d > 0 and i < len(self.keys) - 1:
            return k, self.keys[i + 1]
        return (self.keys[i - 1], k) if d < 0 and i > 0 else None

    def stacked(self, t, chain):
        """A gap's chain in `t` [between, ...]: the forward chain's frame a + s is row first + s - 1, the backward chain's frame
        b - s is row first + length - s."""
        _, _, d, length = chain
        row = t.stride(0) * t.element_size()
        return t.data_ptr() + (self.first[self.of(chain)] + (-1 if d > 0 else length)) * row, d * row

    @staticmethod
    def in_place(t, chain):
        """Frame k + d s is row k + d s of `t` [F, ...]: a gap's forward chain or an edge chain in one of the call's outputs."""
        _, k, d, _ = chain
        row = t.stride(0) * t.element_size()
        return t.data_ptr() + k * row, d * row

    @staticmethod
    def fixed(t, r):
        """Every step at row `r` of `t`: what only the next launch reads."""
        return t[r].data_ptr(), 0


def _linear(column):
    """A column of per-chain (address, byte step) as two int64 arrays."""
    return np.array([c[0] for c in column], dtype=np.int64), np.array([c[1] for c in column], dtype=np.int64)


class Chains:
    """What outlives a step of the chains of a call, and the job tables of a step's launches.  A table is a host uint64 array of
    device addresses; step s of chain c reads and writes at addresses that are linear in s or alternate with its parity, so a
    step fills columns with a few numpy operations and allocates nothing on the device.  `outs`: per chain the (address, byte
    step) of where step s writes its mask.  The occlusion-aware form is an option, off by default, handed in by the module that
    owns it: `split` = (occlusion, mask, hidden, flags, counts), the last four per-chain (address, byte step) columns of where
    step s writes the visible part, the hidden part, the block flags and the number of visible bits (address 0: not counted);
    `outs` then says where the advance's code goes.  With it a group's launches are the walk, the advance, lp_prop_visible_batch
    and lp_prop_occlude_batch; without it, the walk and the advance.  Which buffer serves what:
      - `pos` and `mpyr`, two position maps and two mask pyramids per chain, alternate with the step's parity: step s reads
        [(s - 1) & 1] and writes [s & 1]; step 1 reads a null position map (the key frame's) and the key's own pyramid;
      - the advance writes the pyramid of its mask's bits to mpyr[s & 1], the next step's weights.  With the option it writes
        it to `raw_mpyr`, a buffer per chain that comes with the option, where the flags read the bits; occlude then writes the
        next step's weights, the visible part's bits, to mpyr[s & 1], never to raw_mpyr;
      - the fields are scratch within a step: they are the rows of a `FieldWalk`, which belong to the j-th chain of the group
        being launched, not to a chain of the plan;
      - the key frame's luma is level 0 of its pyramid in `pyr`, which the clip holds whole;
      - `count_keys` runs the occlude launch before step 1 and needs three outputs per chain that nobody reads: it scribbles on
        pos[0], on mpyr[0] and on the chain's `hidden` base address.  Step 1 reads none of them (its positions are null, its
        weights the key's) and writes pos[1] and mpyr[1]; step 2 overwrites pos[0] and mpyr[0] before step 3 reads them; and
        the hidden base, address + 0 * step, is a fixed scratch row that every step's occlude rewrites (a gap's chain; only
        gaps' chains are counted).
    The plain form allocates no raw_mpyr, no visible or occlude table and no descriptor for them.
    The anchored form is the second option, off by default: `rematch` = (anchor,), propagate_keys_anchored's.  With it a group's
    launches are the walk, a first advance, lp_prop_match_batch in its warped-key form, lp_prop_fill_batch and the advance proper
    along that correction, 2 levels + 4.  It comes with `raw_pos` and `raw_mpyr`, a buffer per chain each, where the first advance
    writes the positions and the bits the re-match reads, and with a second advance table and the re-match's descriptor:
      - the first advance's mask goes to the step's output address, which the second advance rewrites;
      - the re-match writes the walk's level-0 raw and valid rows, the fill its level-0 table as the walk left it: the step's own
        field is spent by the first advance;
      - the second advance reads raw_pos and writes pos[s & 1], the output and mpyr[s & 1], as the plain step's one advance does.
    `rematch` with `split` raises: an occluded block needs the gate.
    Both options at once are spelled `rematch` = (anchor, occlusion) next to `split`, propagate_keys_anchored_visible's; the same
    pair without `split` raises, and so does an occlusion that is not split's.  The re-match is then lp_prop_match_batch in its
    gated form and a group's launches are the walk, the first advance, the gated re-match, the fill, the second advance,
    lp_prop_visible_batch and lp_prop_occlude_batch, 2 levels + 6.  No buffer is added to the two options':
      - the first advance writes raw_pos and raw_mpyr, which the gated re-match reads, and its code to the step's code address;
      - the second advance reads raw_pos and writes pos[s & 1], the code to the same address and its bits to raw_mpyr again (the
        re-match has read the first bits by then: the launches are in stream order), where the flags read them;
      - visible and occlude are the split's: occlude writes mask, hidden, the next step's weights to mpyr[s & 1] and the count;
      - `count_keys` scribbles where it did: step 1 reads neither pos[0] nor mpyr[0] and writes raw_pos, raw_mpyr, pos[1], mpyr[1]."""

    def __init__(self, plan, pyr, key_pyrs, outs, H, W, levels, search, smooth, split=None, rematch=None):
        gate = 0                                                     # the re-match's occlusion: above 0 with both options only
        if rematch and len(rematch) > 2:
            raise ValueError(f"rematch must be (anchor,) or (anchor, occlusion), got {rematch!r}")
        if rematch and len(rematch) == 2:
            if not split:
                raise ValueError("rematch=(anchor, occlusion) without split: the gated re-match belongs to the occlusion-aware chains")
            gate = int_in(rematch[1], 1, 255, "rematch's occlusion")
            if gate != split[0]:
                raise ValueError(f"rematch's occlusion {gate} is not split's {split[0]}: a chain has one")
        elif split and rematch:
            raise ValueError("rematch with split: an occluded block would be matched against the occluder, and the batched re-match "
                             "has no gate; rematch=(anchor, occlusion) is the gated one")
        dev = pyr.device
        self.dev = dev
        self.length = np.array([c[3] for c in plan], dtype=np.int64)
        stride = pyr.shape[1]
        self.walk = FieldWalk(min(len(plan), MAX_JOBS), H, W, levels, search, smooth, dev)
        self._keep = []                                              # the device buffers behind the addresses
        self.pos = [self._buffers((H, W, 2), torch.int32) for _ in range(2)]
        self.mpyr = [self._buffers((stride,), torch.uint8) for _ in range(2)]
        self.key = np.array([key_pyrs[c[0]].data_ptr() for c in plan], dtype=np.uint64)
        # frame k + d s of the clip's pyramids, and where step s writes: both base + s * step, the step signed
        self.luma = _linear([(pyr.data_ptr() + c[1] * stride, c[2] * stride) for c in plan])
        self.out = _linear(outs)
        m = len(self.walk.field0)
        self.t_advance = np.zeros((m, 6), dtype=np.uint64)
        self.t_advance[:, 0] = self.walk.field0
        self.launches = [("lp_prop_advance_batch", _cabi.LpPropAdvanceBatchDesc(H, W, levels, 0, self.t_advance.ctypes.data))]
        self.lin = None
        tail = []                                                    # the split's two launches: behind the re-match's, if any
        if split:
            occlusion, *columns = split
            self.raw_mpyr = self._buffers((stride,), torch.uint8)
            self.lin = [_linear(column) for column in columns]
            self.t_visible, self.t_occlude = np.zeros((m, 5), dtype=np.uint64), np.zeros((m, 6), dtype=np.uint64)
            self.occlude_desc = _cabi.LpPropOccludeBatchDesc(H, W, levels, 0, self.t_occlude.ctypes.data)
            tail = [("lp_prop_visible_batch", _cabi.LpPropVisibleBatchDesc(H, W, occlusion, 0, self.t_visible.ctypes.data)),
                    ("lp_prop_occlude_batch", self.occlude_desc)]
        self.rematch = bool(rematch)
        if rematch:
            anchor = int_in(rematch[0], 1, MAX_SEARCH, "anchor")
            self.raw_pos = self._buffers((H, W, 2), torch.int32)
            if not split:                                            # with both options the split's raw_mpyr serves both advances
                self.raw_mpyr = self._buffers((stride,), torch.uint8)
            self.t_rematch, self.t_second = np.zeros((m, 6), dtype=np.uint64), np.zeros((m, 6), dtype=np.uint64)
            self.t_rematch[:, 4], self.t_rematch[:, 5] = self.walk.t_match[0][:, 4], self.walk.t_match[0][:, 5]
            self.t_second[:, 0] = self.walk.field0
            form = _cabi.LP_PROP_MATCH_GATED(gate) if gate else _cabi.LP_PROP_MATCH_WARPED_KEY
            warped = _cabi.LpPropMatchBatchDesc(H, W, levels, 0, anchor, smooth, 0, form, self.t_rematch.ctypes.data)
            # a fill has no descriptor: None stands for the one on the walk's own level-0 table
            self.launches += [("lp_prop_match_batch", warped), ("lp_prop_fill_batch", None),
                              ("lp_prop_advance_batch", _cabi.LpPropAdvanceBatchDesc(H, W, levels, 0, self.t_second.ctypes.data))]
        self.launches += tail

    def _buffers(self, shape, dtype):
        """One buffer of `shape` per chain: their addresses."""
        self._keep.append(torch.empty((len(self.length), *shape), dtype=dtype, device=self.dev))
        return row_addresses(self._keep[-1], len(self.length))

    def step(self, s):
        """Step s of every chain that has one: 2 levels + 1 launches per MAX_JOBS chains, + 2 with `split`, + 3 with `rematch`,
        + 5 with both."""
        idx = np.flatnonzero(self.length >= s)
        for lo in range(0, len(idx), MAX_JOBS):
            self._bind(s, idx[lo:lo + MAX_JOBS])
            self._launch(min(MAX_JOBS, len(idx) - lo))

    def _bind(self, s, idx):
        """The tables' rows 0 .. len(idx) - 1 for step s of the chains `idx`, one group."""
        n = len(idx)

        def at(lin, s=s):
            return (lin[0][idx] + s * lin[1][idx]).astype(np.uint64)
        luma = at(self.luma)                                         # the frame the step arrives at
        self.jobs = (at(self.luma, s - 1), luma, self.key[idx] if s == 1 else self.mpyr[(s - 1) & 1][idx])
        a = self.t_advance
        a[:n, 1] = 0 if s == 1 else self.pos[(s - 1) & 1][idx]
        a[:n, 2], a[:n, 3], a[:n, 4] = self.key[idx], self.pos[s & 1][idx], at(self.out)
        a[:n, 5] = self.raw_mpyr[idx] if self.lin else self.mpyr[s & 1][idx]
        if self.lin:
            mask, hidden, flags, count = map(at, self.lin)
            v, o = self.t_visible, self.t_occlude
            v[:n, 0], v[:n, 1], v[:n, 2], v[:n, 3], v[:n, 4] = a[:n, 3], luma, at(self.luma, 0), a[:n, 5], flags
            o[:n, 0], o[:n, 1], o[:n, 2], o[:n, 3], o[:n, 4], o[:n, 5] = a[:n, 4], flags, mask, hidden, self.mpyr[s & 1][idx], count
        if self.rematch:
            r, b = self.t_rematch, self.t_second
            b[:n, 1], b[:n, 2], b[:n, 3], b[:n, 4], b[:n, 5] = self.raw_pos[idx], a[:n, 2], a[:n, 3], a[:n, 4], a[:n, 5]
            a[:n, 3], a[:n, 5] = self.raw_pos[idx], self.raw_mpyr[idx]
            r[:n, 0], r[:n, 1], r[:n, 2], r[:n, 3] = at(self.luma, 0), luma, a[:n, 5], a[:n, 3]

    def _launch(self, n):
        """The launches of the group of `n` chains that was bound."""
        self.walk.run(*self.jobs)
        for entry, desc in self.launches:
            if desc is None:
                launch(entry, self.dev, self.walk.t_fill[0].ctypes.data, n, *self.walk.grids[0])
                continue
            desc.jobs = n
            launch(entry, self.dev, ctypes.byref(desc))

    def count_keys(self, painted, zero_flags):
        """With the option, before step 1: entry 0 of every counted chain's counts, the key's bits, counted by the occlude launch
        on the key's binarised mask with no block flagged, through the occlude table in groups of MAX_JOBS.  `painted`: per
        chain the key's fp32 bits.  What it writes besides is scribbled where the class's docstring says."""
        (_, (hidden, _), _, (count, _)), pos, mpyr = self.lin, self.pos[0], self.mpyr[0]
        rows = [(painted[c].data_ptr(), zero_flags.data_ptr(), int(pos[c]), int(hidden[c]), int(mpyr[c]), int(count[c]))
                for c in np.flatnonzero(count)]
        table = np.array(rows, dtype=np.uint64).reshape(len(rows), 6)
        for lo in range(0, len(rows), MAX_JOBS):
            n = self.occlude_desc.jobs = min(MAX_JOBS, len(rows) - lo)
            self.t_occlude[:n] = table[lo:lo + n]
            launch("lp_prop_occlude_batch", self.dev, ctypes.byref(self.occlude_desc))


def painted_masks(masks, keys, F, H, W):
    """The K key masks of `masks` ([K, H, W], [F, H, W] or, for one key, [H, W]) as a list of [H, W] tensors; the per-shot form
    (shots.py) picks a shot's keys out of it."""
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
    for k, m in zip(keys, painted_masks(masks, keys, F, H, W)):
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
    gaps = Gaps(keys)
    back = torch.empty((gaps.between, H, W), dtype=torch.float32, device=dev)
    outs = [gaps.stacked(back, c) if c[2] < 0 and gaps.of(c) else gaps.in_place(out, c) for c in plan]
    pyr = clip_pyramids(images, levels)
    chains = Chains(plan, pyr, key_pyrs, outs, H, W, levels, search, smooth)
    for s in range(1, int(chains.length.max()) + 1):
        chains.step(s)
    for a, b in gaps.pairs:
        mid, r = out[a + 1:b], gaps.first[a, b]
        merge_gap(stabilize.signed_d2(mid), stabilize.signed_d2(back[r:r + b - a - 1]), b - a, 1, mid)
    return out
