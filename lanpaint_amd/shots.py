"""Video shot detect: where a clip's hard cuts are, and the temporal links of the video chain run shot by shot.

Every temporal link -- `propagate_masks`, `stabilize_masks`, `temporal_fill`, `temporal_fill_checked`, `temporal_smooth` -- takes
a clip as one continuous shot.  Footage handed to a workflow is often an edit of several.  Across a hard cut the block matcher
still returns a field, and that field means nothing: the temporal fill pastes pixels of the other shot as "known", the smooth
walks into the other shot, the stabilize takes medians over two scenes, a propagated mask runs on into a scene without the
subject.  This module gives the boundary signal and a way to run each link inside a shot:

    video -> detect_shots -> shot_ranges -> *_shots(..., ranges)

shot_scores(images, level=2, search=2) -> (score int64 [F - 1, 2], n_pixels)
        Per pair of neighbouring frames, on level `level` of the 8-bit luma pyramid (`propagate.luma_pyramids`): A, the residual
        that a block matching of 8 x 8 blocks over +-`search` pixels leaves, summed over the plane, and B, the L1 distance of the
        two 64-bin histograms.  `n_pixels` is the plane's size, a Python integer.
shot_decide(score, n_pixels, threshold=16, hist=30, ratio=200, window=4) -> shot int32 [F]
        Pair t is a cut when its mean residual A / n_pixels is at least `threshold` grey levels, at least `hist` percent of the
        pixels change their histogram bin, and 100 A[t] >= ratio A[u] for every other pair u within `window` pairs.  The last
        condition keeps a flash (two high pairs in a row), a run of fast motion and a large object that moves further than the
        search from being called cuts.  It also makes `window` the shortest shot that can be told apart: two cuts closer than
        `window` suppress one another, unless one residual is `ratio` percent of the other.  shot[f] counts the cuts in front
        of frame f.  The defaults of `threshold` and `hist` were chosen on synthetic clips only (profiles/r34_shots.md): low-pass
        canvases that pan under noise, at the default `level` and `search`; no real footage was at hand.
detect_shots(images, ...) -> (shot, score)        the two together.
shot_ranges(shot) -> [(lo, hi), ...]              the frames of every shot: the one device -> host read (F int32 values).
per_shot(fn, ranges, clips, *args, frame_outputs=(), **kw)
        `fn(*clips, *args, **kw)` once per range, with every tensor of `clips` that has one entry per frame cut to the range,
        the outputs joined along the frames; see the function.
temporal_fill_shots, temporal_fill_checked_shots, temporal_smooth_shots, stabilize_masks_shots, propagate_masks_shots
        The five links run per shot; each takes the ranges, or the `shot` tensor, behind the clip.
temporal_smooth_robust_shots
        `temporal_smooth_robust`, the robust form of the smooth, per shot in the same way.
propagate_masks_anchored_shots
        `propagate_masks_anchored`, the anchored form of the propagate, inside the key frame's shot as `propagate_masks_shots`.
propagate_masks_anchored_visible_shots
        `propagate_masks_anchored_visible`, the anchored occlusion-aware form, in the same way: both outputs 0 outside that shot.
propagate_keys_anchored_visible_shots
        `propagate_keys_anchored_visible` per shot on the keys inside it, 0 in a shot without a key.  With anchor = 0 and / or
        occlusion = 0 it is the per-shot form of the three other several-keys propagates, which have none of their own.

include/lanpaint_hip.h (lp_shot_*) states the rule in full: integers throughout, the same bits on every run.  Not done:
dissolves, fades and wipes are not detected; the several-key propagates (but through propagate_keys_anchored_visible_shots) and
the colour match's pooling over neighbouring frames have no shot-aware form.

HIP tensors only, no CPU fallback.  The pyramids are built for as many frames at a time as stay under WS_CAP_BYTES; neighbouring
chunks share one frame, so every pair is measured inside one chunk, and a pair's scores depend on its two frames only: chunking
cannot change a bit.  One measuring launch per chunk (lp_shot_measure), one deciding launch per clip (lp_shot_decide).
"""
from __future__ import annotations

import ctypes

import torch

from . import _cabi
from ._hostcall import chunks, int_in, launch, tensor_is
from ._motion import check_images, luma_pyramids

MAX_LEVEL = _cabi.LP_PROP_MAX_LEVELS - 1
MAX_SEARCH = _cabi.LP_SHOT_MAX_SEARCH
MAX_WINDOW = _cabi.LP_SHOT_MAX_WINDOW
MAX_FRAMES = 65535
THRESHOLD, HIST = 16, 30               # chosen on synthetic clips only: profiles/r34_shots.md
WS_CAP_BYTES = 1 << 30


def _decision(threshold, hist, ratio, window):
    int_in(threshold, 1, 255, "threshold")
    int_in(hist, 0, 100, "hist")
    int_in(ratio, 100, 10000, "ratio")
    int_in(window, 1, MAX_WINDOW, "window")


def measure_planes(planes, stride, frames, h, w, search, score):
    """The measuring launch: `planes` uint8, frame 0's plane first and every further frame's `stride` bytes on; the scores of the
    frames - 1 pairs go to `score` int64 [frames - 1, 2].  Returns the histograms int32 [frames, 64]."""
    hist = torch.empty((frames, _cabi.LP_SHOT_BINS), dtype=torch.int32, device=planes.device)
    d = _cabi.LpShotMeasureDesc(frames, h, w, search, planes.data_ptr(), stride, hist.data_ptr(), score.data_ptr() if frames > 1 else None)
    launch("lp_shot_measure", planes.device, ctypes.byref(d))
    return hist


def shot_scores(images, level=2, search=2):
    """(score int64 [F - 1, 2] on the images' device: A and B of every pair, n_pixels: the plane's size).  No device -> host
    read."""
    int_in(level, 0, MAX_LEVEL, "level")
    int_in(search, 1, MAX_SEARCH, "search")
    check_images(images)
    F, H, W, C = images.shape
    int_in(F, 1, MAX_FRAMES, "the frame count")
    h, w = _cabi.prop_level_shape(H, W, level)
    score = torch.empty((F - 1, 2), dtype=torch.int64, device=images.device)
    stride = _cabi.prop_pyramid_ws_bytes(1, H, W, level + 1)
    per_frame = stride + (0 if images.dtype == torch.float32 else H * W * C * 4)
    off = _cabi.prop_level_offset(H, W, level)
    for s, n in chunks(F - 1, per_frame, max(WS_CAP_BYTES - per_frame, 1)):      # the pairs s .. s + n - 1: n + 1 frames
        pyr = luma_pyramids(images[s:s + n + 1], level + 1)
        measure_planes(pyr[0, off:], stride, n + 1, h, w, search, score[s:s + n])
    return score, h * w


def shot_decide(score, n_pixels, threshold=THRESHOLD, hist=HIST, ratio=200, window=4):
    """`score` int64 [F - 1, 2] -> shot int32 [F] on its device (module docstring).  No device -> host read."""
    _decision(threshold, hist, ratio, window)
    int_in(n_pixels, 1, 1 << 28, "n_pixels")
    tensor_is(score, torch.int64, (None, 2), "score", __name__)
    F = int_in(score.shape[0] + 1, 1, MAX_FRAMES, "the frame count")
    shot = torch.empty((F,), dtype=torch.int32, device=score.device)
    d = _cabi.LpShotDecideDesc(F, threshold, hist, ratio, window, 0, n_pixels, score.data_ptr() if F > 1 else None, shot.data_ptr())
    launch("lp_shot_decide", score.device, ctypes.byref(d))
    return shot


def detect_shots(images, threshold=THRESHOLD, hist=HIST, ratio=200, window=4, level=2, search=2):
    """(shot int32 [F], score int64 [F - 1, 2]) of the clip `images` [F, H, W, C] (module docstring).  No device -> host read."""
    _decision(threshold, hist, ratio, window)
    score, n = shot_scores(images, level, search)
    return shot_decide(score, n, threshold, hist, ratio, window), score


def shot_ranges(shot):
    """`shot` [F], not decreasing -> [(lo, hi), ...], the frames lo .. hi - 1 of every shot.  The one device -> host read of the
    feature: F int32 values."""
    if not torch.is_tensor(shot) or shot.ndim != 1 or shot.shape[0] < 1:
        raise ValueError("shot must be a tensor [F] with at least one frame")
    ids = shot.tolist()
    edges = [0] + [f for f in range(1, len(ids)) if ids[f] != ids[f - 1]] + [len(ids)]
    return list(zip(edges[:-1], edges[1:]))


def _ranges(shots):
    """`shots` as ranges: a `shot` tensor is read, a list of ranges is checked to cover its frames in order."""
    ranges = shot_ranges(shots) if torch.is_tensor(shots) else [(int(lo), int(hi)) for lo, hi in shots]
    if not ranges or ranges[0][0] != 0 or any(hi <= lo for lo, hi in ranges) or any(a[1] != b[0] for a, b in zip(ranges, ranges[1:])):
        raise ValueError(f"the ranges must cover the clip's frames from 0 on, in order and without a gap, got {ranges}")
    return ranges


def per_shot(fn, ranges, clips, *args, frame_outputs=(), **kw):
    """`fn(*clips, *args, **kw)` once per range (lo, hi) of `ranges`.  The frame count F is where the ranges end.  Every tensor of
    `clips` with three or more dimensions whose first is F is cut to [lo:hi]; the others -- a [1, H, W] or [H, W] mask, None --
    go in whole.  `fn` returns a tensor or a tuple of tensors with the range's frames first; each is joined along the frames.
    The outputs whose positions `frame_outputs` lists hold frame indices (`source` of the two fills): `lo` is added where the
    value is >= 0, so -1 and -2 stay.  A single range returns exactly what `fn` returns on the whole clip."""
    ranges = _ranges(ranges)
    F = ranges[-1][1]
    if len(ranges) == 1:
        return fn(*clips, *args, **kw)
    parts = []
    for lo, hi in ranges:
        cut = [c[lo:hi] if torch.is_tensor(c) and c.ndim >= 3 and c.shape[0] == F else c for c in clips]
        out = fn(*cut, *args, **kw)
        single = torch.is_tensor(out)
        out = [out] if single else list(out)
        for i in frame_outputs:
            out[i] = torch.where(out[i] >= 0, out[i] + lo, out[i])
        parts.append(out)
    joined = [torch.cat(column, dim=0) for column in zip(*parts)]
    return joined[0] if single else tuple(joined)


def clip_ranges(shots, frames):
    ranges = _ranges(shots)
    if ranges[-1][1] != frames:
        raise ValueError(f"the shots end at frame {ranges[-1][1]}, the clip has {frames}")
    return ranges


def temporal_fill_shots(images, mask, shots, levels=4, search=2, smooth=8, reach=0):
    """`temporal_fill` inside every shot: nothing is borrowed across a cut.  (filled, remaining, source), `source` in the clip's
    frame numbers.  `shots`: the ranges, or the `shot` tensor (then read here)."""
    from .temporal_fill import temporal_fill
    return per_shot(temporal_fill, clip_ranges(shots, images.shape[0]), (images, mask), levels, search, smooth, reach, frame_outputs=(2,))


def temporal_fill_checked_shots(images, mask, shots, levels=4, search=2, smooth=8, reach=0, agree=8):
    """`temporal_fill_checked` inside every shot: (filled, remaining, source, witnesses)."""
    from .temporal_fill_checked import temporal_fill_checked
    return per_shot(temporal_fill_checked, clip_ranges(shots, images.shape[0]), (images, mask), levels, search, smooth, reach, agree,
                    frame_outputs=(2,))


def temporal_smooth_shots(images, mask, shots, radius=2, tolerance=24, motion="background", levels=4, search=2, smooth=8):
    """`temporal_smooth` inside every shot: no chain walks across a cut.  (out, support)."""
    from .temporal_smooth import temporal_smooth
    return per_shot(temporal_smooth, clip_ranges(shots, images.shape[0]), (images, mask), radius, tolerance, motion, levels, search, smooth)


def temporal_smooth_robust_shots(images, mask, shots, radius=2, tolerance=24, motion="background", levels=4, search=2, smooth=8):
    """`temporal_smooth_robust` inside every shot: no chain walks across a cut and no median is taken over two scenes.
    (out, support, replaced)."""
    from .temporal_smooth_robust import temporal_smooth_robust
    return per_shot(temporal_smooth_robust, clip_ranges(shots, images.shape[0]), (images, mask), radius, tolerance, motion, levels, search,
                    smooth)


def stabilize_masks_shots(mask, shots, median=1, smooth=2, grow=0.0, feather=0.0):
    """`stabilize_masks` inside every shot: no median or mean over two scenes.  `mask` [F, H, W]."""
    from .stabilize import stabilize_masks
    if not torch.is_tensor(mask) or mask.ndim != 3:
        raise ValueError("mask must be [F, H, W]")
    return per_shot(stabilize_masks, clip_ranges(shots, mask.shape[0]), (mask,), median, smooth, grow, feather)


def _in_key_shot(fn, images, mask, shots, key_frame, *args):
    """A single-key propagate `fn(images, mask, key_frame, *args)` inside the key frame's shot; exactly 0 in every other shot.
    `fn` returns one fp32 [F, H, W] or a tuple of them; so does this."""
    check_images(images)
    F = images.shape[0]
    ranges = clip_ranges(shots, F)
    int_in(key_frame, 0, F - 1, "key_frame")
    lo, hi = next(r for r in ranges if r[0] <= key_frame < r[1])
    if len(ranges) == 1:
        return fn(images, mask, key_frame, *args)
    per_frame = torch.is_tensor(mask) and mask.ndim == 3 and mask.shape[0] == F
    part = fn(images[lo:hi], mask[lo:hi] if per_frame else mask, key_frame - lo, *args)
    outs = []
    for p in part if isinstance(part, tuple) else (part,):
        out = torch.zeros(tuple(images.shape[:3]), dtype=torch.float32, device=images.device)
        out[lo:hi] = p
        outs.append(out)
    return tuple(outs) if isinstance(part, tuple) else outs[0]


def propagate_masks_shots(images, mask, shots, key_frame=0, levels=4, search=2, smooth=8):
    """`propagate_masks` inside the key frame's shot; exactly 0 in every other shot: the subject of one scene is not in the next.
    fp32 [F, H, W]."""
    from .propagate import propagate_masks
    return _in_key_shot(propagate_masks, images, mask, shots, key_frame, levels, search, smooth)


def propagate_masks_anchored_shots(images, mask, shots, key_frame=0, levels=4, search=2, smooth=8, anchor=2):
    """`propagate_masks_anchored` inside the key frame's shot; exactly 0 in every other shot.  fp32 [F, H, W]."""
    from .propagate_anchored import propagate_masks_anchored
    return _in_key_shot(propagate_masks_anchored, images, mask, shots, key_frame, levels, search, smooth, anchor)


def propagate_masks_anchored_visible_shots(images, mask, shots, key_frame=0, levels=4, search=2, smooth=8, anchor=2, occlusion=16):
    """`propagate_masks_anchored_visible` inside the key frame's shot; `mask` and `hidden` exactly 0 in every other shot.
    (fp32 [F, H, W], fp32 [F, H, W])."""
    from .propagate_anchored_visible import propagate_masks_anchored_visible
    return _in_key_shot(propagate_masks_anchored_visible, images, mask, shots, key_frame, levels, search, smooth, anchor, occlusion)


def propagate_keys_anchored_visible_shots(images, masks, shots, key_frames, levels=4, search=2, smooth=8, anchor=2, occlusion=16):
    """`propagate_keys_anchored_visible` inside every shot, on the keys that lie inside it: no chain runs across a cut and no
    merge joins the keys of two scenes.  A shot without a key is exactly 0 in both outputs; a single range returns the plain
    call's result.  `masks` as the call takes them, [K, H, W], [F, H, W] or [H, W] for one key.  With anchor = 0 and / or
    occlusion = 0 this is the per-shot form of `propagate_keys_visible`, `propagate_keys_anchored` (and zeros) and
    `propagate_keys` (and zeros) as well.  (fp32 [F, H, W], fp32 [F, H, W])."""
    from .propagate_keys import chain_plan, painted_masks
    from .propagate_keys_anchored_visible import propagate_keys_anchored_visible
    if not torch.is_tensor(images) or images.ndim != 4:
        check_images(images)                                         # raises; every other check of the clip is the call's own
    F, H, W = images.shape[:3]
    ranges = clip_ranges(shots, F)
    chain_plan(F, key_frames)                                        # the keys' own checks, before anything is cut
    keys = list(key_frames)
    if len(ranges) == 1:
        return propagate_keys_anchored_visible(images, masks, keys, levels, search, smooth, anchor, occlusion)
    if not torch.is_tensor(masks):
        raise ValueError("masks must be a tensor [K, H, W], [F, H, W] or [H, W]")
    painted = painted_masks(masks, keys, F, H, W)
    out = torch.zeros((F, H, W), dtype=torch.float32, device=images.device)
    hidden = torch.zeros_like(out)
    for lo, hi in ranges:
        inside = [i for i, k in enumerate(keys) if lo <= k < hi]
        if inside:
            out[lo:hi], hidden[lo:hi] = propagate_keys_anchored_visible(
                images[lo:hi], torch.stack([painted[i] for i in inside]), [keys[i] - lo for i in inside], levels, search, smooth,
                anchor, occlusion)
    return out, hidden
