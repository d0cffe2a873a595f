"""LanPaint_VideoShots and the shot-aware video nodes: find the hard cuts of a clip and run the temporal nodes shot by shot.

The video mask propagate, the mask stabilize, the two temporal fills and the temporal smooth take a clip as one continuous shot.
A video handed to a workflow is often an edit of several, and across a hard cut every one of them mixes two scenes.
LanPaint_VideoShots (lanpaint_amd.shots, on the HIP device) finds the cuts; LanPaint_VideoShotSelect cuts one shot out of a clip
for any node; and a subclass of each of the five temporal nodes takes the `shots` and works inside every shot on its own:

    video -> VideoShots -> (shots) VideoMaskPropagateShots -> VideoMaskStabilizeShots -> VideoTemporalFillShots -> ...
                                   ... -> VideoTemporalSmoothShots

Hard cuts only: dissolves, fades and wipes are not detected.  Two cuts closer than `window` frames suppress one another.  The
several-key propagate nodes (but LanPaint_VideoMaskPropagateKeysAnchoredVisibleShots, in its own module, which with its options
off is each of them) and the colour match's pooling over neighbouring frames have no shot-aware form.  Host tensors in
and out like the other nodes.  The reference has no such nodes.

This module has its own NODE_CLASS_MAPPINGS: merge them with the others' (INTEGRATION.md section 2(b)).
"""
from __future__ import annotations

import torch

from . import shots as _shots
from ._hostcall import node_device
from .propagate_nodes import LanPaint_VideoMaskPropagate
from .stabilize_nodes import LanPaint_VideoMaskStabilize
from .temporal_fill_checked_nodes import LanPaint_VideoTemporalFillChecked
from .temporal_fill_nodes import LanPaint_VideoTemporalFill
from .temporal_smooth_nodes import LanPaint_VideoTemporalSmooth

SHOTS_TYPE = "LANPAINT_SHOTS"          # the host list of ranges [(lo, hi), ...]


class LanPaint_VideoShots:
    """Find the hard cuts of a video: the frames of every shot."""

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {
            "image": ("IMAGE", {"tooltip": "The video, one frame per batch entry."}),
            "threshold": ("INT", {"default": _shots.THRESHOLD, "min": 1, "max": 255, "step": 1,
                                  "tooltip": "The least mean residual of a cut, in grey levels (of 255), that a block matching "
                                             "between the two frames leaves. Chosen on synthetic clips only."}),
            "hist": ("INT", {"default": _shots.HIST, "min": 0, "max": 100, "step": 1,
                             "tooltip": "The least share of the pixels, in percent, that change their bin of a 64-bin brightness "
                                        "histogram across a cut. Chosen on synthetic clips only."}),
            "ratio": ("INT", {"default": 200, "min": 100, "max": 10000, "step": 10,
                              "tooltip": "A cut's residual must be this many percent of every other residual within `window` "
                                         "frames: keeps a flash, fast motion and a large fast object from being called cuts."}),
            "window": ("INT", {"default": 4, "min": 1, "max": _shots.MAX_WINDOW, "step": 1,
                               "tooltip": "The frames on either side a cut is compared with. It is the shortest shot that can be "
                                          "told apart: two cuts closer than this suppress one another."}),
            "level": ("INT", {"default": 2, "min": 0, "max": _shots.MAX_LEVEL, "step": 1,
                              "tooltip": "The pyramid level measured on: every level halves the picture. Coarser is faster and "
                                         "forgives more motion."}),
            "search": ("INT", {"default": 2, "min": 1, "max": _shots.MAX_SEARCH, "step": 1,
                               "tooltip": "Pixels of that level searched for a block's motion before its residual is taken."}),
        }}

    RETURN_TYPES = (SHOTS_TYPE, "INT", "STRING")
    RETURN_NAMES = ("shots", "count", "summary")
    FUNCTION = "detect"
    CATEGORY = "image"
    DESCRIPTION = ("Finds the hard cuts of a video: a motion-compensated residual and a histogram change per pair of frames, and a "
                   "cut where both are high and the residual stands out of its neighbours. Give `shots` to the shot-aware video "
                   "nodes, so that no mask, fill or smoothing crosses a cut. `summary` lists the frames of every shot, such as "
                   "0-29, 30-80. Dissolves, fades and wipes are not detected; two cuts closer than `window` frames suppress one "
                   "another.")

    def detect(self, image, threshold=_shots.THRESHOLD, hist=_shots.HIST, ratio=200, window=4, level=2, search=2):
        dev = node_device(image)
        shot, _ = _shots.detect_shots(image.to(dev), int(threshold), int(hist), int(ratio), int(window), int(level), int(search))
        ranges = _shots.shot_ranges(shot)
        return (ranges, len(ranges), ", ".join(f"{lo}-{hi - 1}" for lo, hi in ranges))


def _per_frame(t, frames):
    return torch.is_tensor(t) and t.ndim >= 3 and t.shape[0] == frames


class LanPaint_VideoShotSelect:
    """Cut one shot out of a video and its mask."""

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {
            "image": ("IMAGE", {"tooltip": "The video, one frame per batch entry."}),
            "shots": (SHOTS_TYPE, {"tooltip": "The shots of that video, from LanPaint_VideoShots."}),
            "index": ("INT", {"default": 0, "min": 0, "max": 65534, "step": 1, "tooltip": "Which shot, counted from 0."}),
        }, "optional": {
            "mask": ("MASK", {"tooltip": "A mask per video frame is cut like the video; one mask for every frame passes through."}),
        }}

    RETURN_TYPES = ("IMAGE", "MASK")
    RETURN_NAMES = ("image", "mask")
    FUNCTION = "select"
    CATEGORY = "image"
    DESCRIPTION = ("Cuts shot `index` out of a video, and out of its per-frame mask, for nodes that have no shot-aware form. "
                   "Without a mask an empty one of the shot's size is returned.")

    def select(self, image, shots, index=0, mask=None):
        ranges = _shots.clip_ranges(shots, image.shape[0])
        if not 0 <= int(index) < len(ranges):
            raise ValueError(f"index {index}: the clip has {len(ranges)} shots")
        lo, hi = ranges[int(index)]
        if mask is None:
            mask = torch.zeros((hi - lo, *image.shape[1:3]), dtype=torch.float32, device=image.device)
        return (image[lo:hi], mask[lo:hi] if _per_frame(mask, image.shape[0]) else mask)


class _PerShot:
    """What the five shot-aware nodes share: the `shots` input behind the parent's own, and the parent's node function called
    once per range on the inputs that have one entry per frame, its outputs joined along the frames."""

    @classmethod
    def INPUT_TYPES(s):
        types = {k: dict(v) for k, v in super().INPUT_TYPES().items()}
        types.setdefault("optional", {})["shots"] = (SHOTS_TYPE, {
            "tooltip": "The shots of the video, from LanPaint_VideoShots: the node works inside every shot on its own. "
                       "Without them the clip is one shot."})
        return types

    def _ranges(self, shots, frames):
        return [(0, frames)] if shots is None else _shots.clip_ranges(shots, frames)

    def _per_shot(self, shots, clips, **kw):
        """`clips`: the parent function's frame inputs by name, the video or per-frame mask first."""
        first = next(iter(clips.values()))
        frames = first.shape[0] if first.ndim >= 3 else 1
        fn = getattr(super(), self.FUNCTION)
        return _shots.per_shot(lambda *cut: fn(**dict(zip(clips, cut)), **kw), self._ranges(shots, frames), tuple(clips.values()))

    def _in_key_shot(self, shots, image, mask, key_frame, *args):
        """The single-key propagate nodes: the parent's function on the key frame's shot, every output empty in every other shot."""
        frames, key = image.shape[0], int(key_frame)
        if not 0 <= key < frames:
            raise ValueError(f"key_frame must be in 0..{frames - 1}, got {key_frame}")
        lo, hi = next(r for r in self._ranges(shots, frames) if r[0] <= key < r[1])
        parts = getattr(super(), self.FUNCTION)(image[lo:hi], mask[lo:hi] if _per_frame(mask, frames) else mask, key - lo, *args)
        if (lo, hi) == (0, frames):
            return parts
        outs = tuple(torch.zeros((frames, *part.shape[1:]), dtype=part.dtype, device=part.device) for part in parts)
        for out, part in zip(outs, parts):
            out[lo:hi] = part
        return outs


_NOTE = " With `shots` it works inside every shot on its own, so nothing crosses a hard cut."


class LanPaint_VideoTemporalFillShots(_PerShot, LanPaint_VideoTemporalFill):
    DESCRIPTION = LanPaint_VideoTemporalFill.DESCRIPTION + _NOTE

    def fill(self, image, mask, levels=4, search=2, smooth=8, reach=0, shots=None):
        return self._per_shot(shots, {"image": image, "mask": mask}, levels=levels, search=search, smooth=smooth, reach=reach)


class LanPaint_VideoTemporalFillCheckedShots(_PerShot, LanPaint_VideoTemporalFillChecked):
    DESCRIPTION = LanPaint_VideoTemporalFillChecked.DESCRIPTION + _NOTE

    def fill(self, image, mask, levels=4, search=2, smooth=8, reach=0, agree=8, shots=None):
        return self._per_shot(shots, {"image": image, "mask": mask}, levels=levels, search=search, smooth=smooth, reach=reach,
                              agree=agree)


class LanPaint_VideoTemporalSmoothShots(_PerShot, LanPaint_VideoTemporalSmooth):
    DESCRIPTION = LanPaint_VideoTemporalSmooth.DESCRIPTION + _NOTE

    def smooth(self, image, mask, radius=2, tolerance=24, motion="background", levels=4, search=2, smooth=8, shots=None):
        return self._per_shot(shots, {"image": image, "mask": mask}, radius=radius, tolerance=tolerance, motion=motion, levels=levels,
                              search=search, smooth=smooth)


class LanPaint_VideoMaskStabilizeShots(_PerShot, LanPaint_VideoMaskStabilize):
    DESCRIPTION = LanPaint_VideoMaskStabilize.DESCRIPTION + _NOTE

    def stabilize(self, mask, median_radius=1, smooth_radius=2, grow=0.0, feather=0.0, shots=None):
        return self._per_shot(shots, {"mask": mask}, median_radius=median_radius, smooth_radius=smooth_radius, grow=grow,
                              feather=feather)


class LanPaint_VideoMaskPropagateShots(_PerShot, LanPaint_VideoMaskPropagate):
    DESCRIPTION = (LanPaint_VideoMaskPropagate.DESCRIPTION + " With `shots` the mask is followed inside the key frame's shot and is "
                   "empty in every other shot: the subject of one scene is not in the next.")

    def propagate(self, image, mask, key_frame=0, levels=4, search=2, smooth=8, shots=None):
        return self._in_key_shot(shots, image, mask, key_frame, levels, search, smooth)


NODE_CLASS_MAPPINGS = {
    "LanPaint_VideoShots": LanPaint_VideoShots,
    "LanPaint_VideoShotSelect": LanPaint_VideoShotSelect,
    "LanPaint_VideoTemporalFillShots": LanPaint_VideoTemporalFillShots,
    "LanPaint_VideoTemporalFillCheckedShots": LanPaint_VideoTemporalFillCheckedShots,
    "LanPaint_VideoTemporalSmoothShots": LanPaint_VideoTemporalSmoothShots,
    "LanPaint_VideoMaskStabilizeShots": LanPaint_VideoMaskStabilizeShots,
    "LanPaint_VideoMaskPropagateShots": LanPaint_VideoMaskPropagateShots,
}
NODE_DISPLAY_NAME_MAPPINGS = {
    "LanPaint_VideoShots": "LanPaint Video Shots",
    "LanPaint_VideoShotSelect": "LanPaint Video Shot Select",
    "LanPaint_VideoTemporalFillShots": "LanPaint Video Temporal Fill (Shots)",
    "LanPaint_VideoTemporalFillCheckedShots": "LanPaint Video Temporal Fill (Checked, Shots)",
    "LanPaint_VideoTemporalSmoothShots": "LanPaint Video Temporal Smooth (Shots)",
    "LanPaint_VideoMaskStabilizeShots": "LanPaint Video Mask Stabilize (Shots)",
    "LanPaint_VideoMaskPropagateShots": "LanPaint Video Mask Propagate (Shots)",
}
