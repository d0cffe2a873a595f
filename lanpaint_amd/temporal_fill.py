"""Video temporal fill: what lies under the mask of a frame is borrowed from the nearest frame that shows it.

The video chain makes a mask (`propagate*`, `stabilize`, `refine`) and finishes an inpaint (colour match, stitches, multiband
blend, grain match); under the mask the only fill in front of the encode was `fill.mask_fill`, a per-frame spatial continuation
that invents a blur where, in most clips, the true picture is visible a few frames earlier or later.  This takes it from there:

    mask chain -> temporal_fill -> (remaining mask) mask_fill -> encode / Detailer crops

temporal_fill(images, mask, levels=4, search=2, smooth=8, reach=0) -> (filled, remaining, source)
        `images` [F, H, W, C]; `mask` [F, H, W], [1, H, W] or [H, W] (then the one mask serves every frame), binarised at 0.5.
        The motion of the background from every frame to its two neighbours is the block field of `propagate` (`levels`,
        `search`, `smooth` as there), weighted by the known pixels -- the mask's complement -- and continued across the hole.
        Along it an origin (frame, position in 1/16 pixel) is carried from frame to frame, forwards, then backwards; a masked
        pixel takes the nearer of the two origins in time (a tie stays with the past), at most `reach` frames away (0: the whole
        clip), and is sampled there once, bilinearly, in fp32.  `filled` fp32 [F, H, W, C]: the images with those pixels
        replaced; `remaining` fp32 [F, H, W]: 1.0 where the mask is set and no frame showed the pixel; `source` int32
        [F, H, W]: the frame a pixel came from, the frame itself outside the mask, -1 where it remains.  One frame, an empty or
        a full mask returns the images; a subject that does not move against its background stays in `remaining`; under
        noise-free whole-pixel motion the borrowed pixels are the true background bit for bit; nothing outside the mask changes.
        include/lanpaint_hip.h (lp_tfill_*) states the rule in full.  Not done: colour or exposure matching of what is borrowed
        (DetailerColorMatch exists), motion boundaries finer than a block; the consistency check on it is temporal_fill_checked's.

HIP tensors only, no CPU fallback, no device -> host read.  A step's field depends on its two frames and one mask only, so the
2 (F - 1) fields of a clip are independent jobs of lp_prop_match_batch / lp_prop_fill_batch, 32 to a launch; only the carry, one
light launch per step, is sequential.  Pyramids and fields are built for as many steps at a time as stay under WS_CAP_BYTES; a
field depends on nothing carried, so chunking cannot change a bit.  The fp32 copy of the clip that is sampled and the three
outputs are held whole.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _cabi
from ._hostcall import chunks, int_in, launch, require_hip, tensor_is, workspace
from ._motion import MAX_JOBS, FieldWalk, check_images, check_params, check_plane, clip_mask, luma_pyramids, row_addresses
from ._util import _as_f32c

MAX_REACH = _cabi.LP_TFILL_MAX_REACH
MAX_FRAMES = 65535
WS_CAP_BYTES = 1 << 30


def known_pyramids(mask, frames, levels, source=None, remaining=None, frame0=0):
    """Stage 1 for `mask` [frames, H, W] or [1, H, W] on a HIP device: uint8 [frames, stride], every frame's known-bit pyramid as
    one row (`propagate.level_view` cuts a level out).  With `source` int32 and `remaining` fp32 [frames, H, W] the planes the
    carry starts from are written too; `frame0` is the clip's index of the first of these frames.  1 + (levels - 1) launches
    for all frames."""
    int_in(levels, 1, _cabi.LP_PROP_MAX_LEVELS, "levels")
    int_in(frames, 1, MAX_FRAMES, "frames")
    int_in(frame0, 0, MAX_FRAMES - frames, "frame0")
    require_hip(mask, "mask", __name__)
    if mask.ndim != 3 or mask.shape[0] not in (1, frames):
        raise ValueError(f"mask must be [{frames}, H, W] or [1, H, W], got {tuple(mask.shape)}")
    mask = _as_f32c(mask)
    _, H, W = mask.shape
    check_plane(H, W)
    for t, dtype, what in ((source, torch.int32, "source"), (remaining, torch.float32, "remaining")):
        if t is not None:
            tensor_is(t, dtype, (frames, H, W), what, __name__)
    pyr = workspace(_cabi.load().lp_prop_pyramid_ws_bytes(frames, H, W, levels), mask.device, "lp_prop_pyramid_ws_bytes")
    d = _cabi.LpTfillKnownDesc(frames, H, W, levels, mask.shape[0], frame0, mask.data_ptr(), pyr.data_ptr(),
                               None if source is None else source.data_ptr(), None if remaining is None else remaining.data_ptr())
    launch("lp_tfill_known", mask.device, ctypes.byref(d))
    return pyr.view(frames, -1)


def step_fields(luma, known, steps, H, W, levels, search=2, smooth=8):
    """Stage 2: the level-0 final fields of `steps`, a list of (frame, donor) rows of `luma` and `known` (frame pyramids uint8
    [n, stride]): int32 [len(steps), gh, gw, 2].  Per MAX_JOBS steps 2 levels launches of lp_prop_match_batch / lp_prop_fill_batch;
    what the levels above 0 leave is scratch shared by every group of jobs."""
    check_params(levels, search, smooth)
    check_plane(H, W)
    stride = _cabi.prop_pyramid_ws_bytes(1, H, W, levels)
    tensor_is(luma, torch.uint8, (None, stride), "luma", __name__)
    tensor_is(known, torch.uint8, (None, stride), "known", __name__)
    if known.shape[0] != luma.shape[0]:
        raise ValueError(f"luma holds {luma.shape[0]} frames and known {known.shape[0]}")
    steps = [(int_in(t, 0, luma.shape[0] - 1, "a step's frame"), int_in(s, 0, luma.shape[0] - 1, "a step's donor")) for t, s in steps]
    out = torch.empty((len(steps), *_cabi.prop_grid(H, W), 2), dtype=torch.int32, device=luma.device)
    if not steps:
        return out
    walk = FieldWalk(min(MAX_JOBS, len(steps)), H, W, levels, search, smooth, luma.device, level0=False)
    frame = np.array([t for t, _ in steps], dtype=np.uint64) * np.uint64(stride)
    donor = np.array([s for _, s in steps], dtype=np.uint64) * np.uint64(stride)
    src, tgt, weight = np.uint64(luma.data_ptr()) + frame, np.uint64(luma.data_ptr()) + donor, np.uint64(known.data_ptr()) + frame
    dst = row_addresses(out, len(steps))
    for lo in range(0, len(steps), MAX_JOBS):
        walk.run(src[lo:lo + MAX_JOBS], tgt[lo:lo + MAX_JOBS], weight[lo:lo + MAX_JOBS], dst[lo:lo + MAX_JOBS])
    return out


def new_state(H, W, dev):
    """The state planes of one frame: (org int32 [H, W], pos int32 [H, W, 2]).  Their content matters under the mask only."""
    return torch.empty((H, W), dtype=torch.int32, device=dev), torch.empty((H, W, 2), dtype=torch.int32, device=dev)


def carry_planes(vec, known, donor_known, state, images, filled, source, remaining, out, **more):
    """The planes of a carry, checked: `images` (already checked) gives the shapes, `more` names further int32 [F, H, W] planes.
    Returns the frame's (org, pos): `out`, new when it is None."""
    F, H, W, C = images.shape
    out = new_state(H, W, images.device) if out is None else out
    i32, f32, u8 = torch.int32, torch.float32, torch.uint8
    planes = [(vec, i32, (*_cabi.prop_grid(H, W), 2), "vec"), (known, u8, (H, W), "known"), (donor_known, u8, (H, W), "donor_known"),
              (images, f32, (F, H, W, C), "images"), (filled, f32, (F, H, W, C), "filled"), (source, i32, (F, H, W), "source"),
              (remaining, f32, (F, H, W), "remaining"), *((t, i32, (F, H, W), what) for what, t in more.items()),
              (out[0], i32, (H, W), "the state's org"), (out[1], i32, (H, W, 2), "the state's pos")]
    if state is not None:
        planes += [(state[0], i32, (H, W), "the donor state's org"), (state[1], i32, (H, W, 2), "the donor state's pos")]
    for t, dtype, shape, what in planes:
        tensor_is(t, dtype, shape, what, __name__)
    return out


def carry(vec, known, donor_known, state, images, filled, source, remaining, frame, donor, reach=0, nearer=False, out=None):
    """Stages 3 and 4 for one step of one direction: frame `frame` takes its origins from its neighbour `donor` through the
    step's field `vec`, and its masked pixels that have one are sampled from `images` into `filled`, with `source` and
    `remaining` (`nearer`: only where the origin is nearer in time than what `source` names).  `known`, `donor_known` uint8
    [H, W]; `state` the donor's (org, pos) or None when the donor is the first frame of the direction.  The frame's (org, pos),
    `out` when given.  One launch."""
    int_in(reach, 0, MAX_REACH, "reach")
    F, H, W, C = check_images(images).shape
    int_in(F, 2, MAX_FRAMES, "the frame count")
    int_in(frame, 0, F - 1, "frame")
    int_in(donor, 0, F - 1, "donor")
    if abs(frame - donor) != 1:
        raise ValueError(f"donor {donor} is not a neighbour of frame {frame}")
    out = carry_planes(vec, known, donor_known, state, images, filled, source, remaining, out)
    d = _cabi.LpTfillCarryDesc(F, H, W, C, frame, donor, reach, int(bool(nearer)), vec.data_ptr(), known.data_ptr(),
                               donor_known.data_ptr(), None if state is None else state[0].data_ptr(),
                               None if state is None else state[1].data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                               images.data_ptr(), filled.data_ptr(), source.data_ptr(), remaining.data_ptr())
    launch("lp_tfill_carry", images.device, ctypes.byref(d))
    return out


class Pyramids:
    """The luma and known pyramids of a range of frames, built when another range is asked for.  The first time a frame's known
    bits are built its `source` and `remaining` planes are started with them."""

    def __init__(self, images, mask, levels, source, remaining):
        self.images, self.mask, self.levels, self.source, self.remaining = images, mask, levels, source, remaining
        self.range, self.started, self.luma, self.known = None, 0, None, None

    def _known(self, lo, hi, start):
        mask = self.mask if self.mask.shape[0] == 1 else self.mask[lo:hi]
        return known_pyramids(mask, hi - lo, self.levels, *((self.source[lo:hi], self.remaining[lo:hi], lo) if start else ()))

    def get(self, lo, hi):
        """(luma, known) uint8 [hi - lo, stride] of frames lo .. hi - 1."""
        if self.range != (lo, hi):
            self.luma = self.known = None                                # the last range goes before the next is allocated
            self.luma = luma_pyramids(self.images[lo:hi], self.levels)
            new = min(max(self.started, lo), hi)                         # frames new .. hi - 1 have no start planes yet
            parts = [self._known(a, b, start) for a, b, start in ((lo, new, False), (new, hi, True)) if b > a]
            self.known = parts[0] if len(parts) == 1 else torch.cat(parts)
            self.range, self.started = (lo, hi), max(self.started, hi)
        return self.luma, self.known


def clip_outputs(images, mask, levels):
    """What the two fills start from: (the contiguous fp32 clip that is sampled, `filled`, a copy of it, written next to it,
    remaining fp32 [F, H, W], source int32 [F, H, W], their `Pyramids`).  One frame: its source and remaining are written."""
    check_images(images)
    F, H, W, _ = images.shape
    int_in(F, 1, MAX_FRAMES, "the frame count")
    dev = images.device
    mask = _as_f32c(clip_mask(mask, F, H, W, __name__).to(dev))
    images = _as_f32c(images)
    filled = images.clone()
    source = torch.empty((F, H, W), dtype=torch.int32, device=dev)
    remaining = torch.empty((F, H, W), dtype=torch.float32, device=dev)
    pyramids = Pyramids(images, mask, levels, source, remaining)
    if F == 1:
        pyramids.get(0, 1)
    return images, filled, remaining, source, pyramids


def carry_direction(entry, desc, order, pyramids, states, fields_args, cap):
    """The carries of one direction of a clip, one launch of `entry` per step along the frames `order`: `desc` holds what does
    not move with the step; `states` are the two (org, pos) the steps alternate between; `fields_args` = (H, W, levels, search,
    smooth).  Pyramids and fields are built for as many steps at a time as stay under `cap` bytes."""
    H, W, levels = fields_args[:3]
    stride = _cabi.prop_pyramid_ws_bytes(1, H, W, levels)
    gh, gw = _cabi.prop_grid(H, W)
    per_step = 2 * stride + gh * gw * 8                                  # a frame's two pyramids and a field
    dev = pyramids.images.device
    done = 0                                                             # carries of this direction so far
    for first, n in chunks(len(order) - 1, per_step, max(cap - 2 * stride, 1)):
        lo, hi = min(order[first], order[first + n]), max(order[first], order[first + n]) + 1
        luma, known = pyramids.get(lo, hi)
        fields = step_fields(luma, known, [(order[k] - lo, order[k - 1] - lo) for k in range(first + 1, first + n + 1)], *fields_args)
        for j, k in enumerate(range(first + 1, first + n + 1)):
            t, s = order[k], order[k - 1]
            src, dst = states[(done + 1) & 1], states[done & 1]
            desc.frame, desc.donor, desc.vec = t, s, fields[j].data_ptr()
            desc.known, desc.donor_known = known[t - lo].data_ptr(), known[s - lo].data_ptr()
            desc.org_src, desc.pos_src = (None, None) if done == 0 else (src[0].data_ptr(), src[1].data_ptr())
            desc.org_dst, desc.pos_dst = dst[0].data_ptr(), dst[1].data_ptr()
            launch(entry, dev, ctypes.byref(desc))
            done += 1


def temporal_fill(images, mask, levels=4, search=2, smooth=8, reach=0):
    """What lies under `mask` in the frames `images` [F, H, W, C], borrowed from the nearest frame that shows it (module
    docstring): (filled fp32 [F, H, W, C], remaining fp32 [F, H, W], source int32 [F, H, W]) on the images' device.  No
    device -> host read."""
    check_params(levels, search, smooth)
    int_in(reach, 0, MAX_REACH, "reach")
    images, filled, remaining, source, pyramids = clip_outputs(images, mask, levels)
    F, H, W, C = images.shape
    if F > 1:
        states = [new_state(H, W, images.device) for _ in range(2)]
        desc = _cabi.LpTfillCarryDesc(F, H, W, C, 0, 0, reach, 0, None, None, None, None, None, None, None, images.data_ptr(),
                                      filled.data_ptr(), source.data_ptr(), remaining.data_ptr())
        for order in (list(range(F)), list(range(F - 1, -1, -1))):       # forwards, then backwards: only what is nearer in time
            carry_direction("lp_tfill_carry", desc, order, pyramids, states, (H, W, levels, search, smooth), WS_CAP_BYTES)
            desc.nearer = 1
    return filled, remaining, source
