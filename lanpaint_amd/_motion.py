"""What the motion modules (propagate, propagate_visible, propagate_anchored, propagate_anchored_visible, propagate_keys,
propagate_keys_visible, propagate_keys_anchored, temporal_fill, temporal_fill_checked, temporal_smooth, temporal_smooth_robust, shots) share on top of
_hostcall.py: the checks of the block matcher's numbers and planes, of a frame's planes next to the warped key frame
(`check_frame_planes`), the clip-mask shapes, the luma pyramids, and the batched coarse-to-fine field walk.  Plain
functions and one small class; no nodes, nothing of the engine's path.  HIP tensors only, no CPU fallback.

Who owns which buffer.  A `FieldWalk` owns the scratch of one group of at most LP_PROP_MAX_JOBS jobs: per level the raw field,
its valid flags and (below the caller's own destination) the final field, next to the host tables and descriptors of its
launches.  Nothing in it outlives a `run`; a caller keeps what does: `propagate_keys.Chains` per chain the two position maps,
the two mask pyramids and the addresses of its key, luma and output rows; `temporal_fill.step_fields` the level-0 fields it
returns.  Every module keeps its own WS_CAP_BYTES and hands it in where a function here chunks.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _cabi
from ._hostcall import chunks, int_in, launch, require_hip, tensor_is, workspace
from ._util import _as_f32c

MAX_SIDE = _cabi.LP_VMASK_MAX_SIDE
MAX_LEVELS = _cabi.LP_PROP_MAX_LEVELS
MAX_SEARCH = _cabi.LP_PROP_MAX_SEARCH
MAX_SMOOTH = _cabi.LP_PROP_MAX_SMOOTH
MAX_JOBS = _cabi.LP_PROP_MAX_JOBS


def check_params(levels, search, smooth):
    int_in(levels, 1, MAX_LEVELS, "levels")
    int_in(search, 1, MAX_SEARCH, "search")
    int_in(smooth, 0, MAX_SMOOTH, "smooth")


def check_plane(H, W):
    if min(H, W) < 1 or max(H, W) > MAX_SIDE:
        raise ValueError(f"a {H}x{W} plane: sides 1..{MAX_SIDE}")


def check_images(images):
    require_hip(images, "images", __name__)
    if images.ndim != 4 or min(images.shape) < 1 or images.shape[3] > _cabi.LP_DETAIL_MAX_CHANNELS:
        raise ValueError(f"images must be [F, H, W, C] with 1..{_cabi.LP_DETAIL_MAX_CHANNELS} channels, got {tuple(images.shape)}")
    check_plane(images.shape[1], images.shape[2])
    return images


def check_frame_planes(pos, tgt, key, mask_bits, module, plane=(None, None)):
    """What the stages that hold a frame against the warped key frame take: `tgt`, `key` and `mask_bits` uint8 [H, W] of one
    plane within the limits (of `plane`, where a batch's first job has set it), `pos` int32 [H, W, 2].  (H, W); `module` is the
    caller's __name__."""
    H, W = tensor_is(tgt, torch.uint8, plane, "tgt", module).shape
    check_plane(H, W)
    tensor_is(key, torch.uint8, (H, W), "key", module)
    tensor_is(mask_bits, torch.uint8, (H, W), "mask_bits", module)
    tensor_is(pos, torch.int32, (H, W, 2), "pos", module)
    return H, W


def clip_mask(mask, F, H, W, module):
    """A clip's `mask` on a HIP device, [H, W], [1, H, W] or [F, H, W], as [1 or F, H, W]."""
    require_hip(mask, "mask", module)
    if mask.ndim == 2:
        mask = mask.unsqueeze(0)
    if mask.ndim != 3 or mask.shape[0] not in (1, F) or tuple(mask.shape[1:]) != (H, W):
        raise ValueError(f"mask {tuple(mask.shape)} does not match {F} frames of {H}x{W}: [H, W], [1, H, W] or [F, H, W]")
    return mask


def level_view(pyr, H, W, level):
    """Level `level` of the frame pyramids `pyr` uint8 [n, stride]: a view [n, h_l, w_l]."""
    h, w = _cabi.prop_level_shape(H, W, level)
    off = _cabi.prop_level_offset(H, W, level)
    return pyr[:, off:off + h * w].view(pyr.shape[0], h, w)


def luma_pyramids(images, levels, out=None, cap=None):
    """Stages 1 and 2 for `images` [n, H, W, C] on a HIP device: uint8 [n, stride], every frame's luma pyramid as one row
    (`level_view` cuts a level out).  1 + (levels - 1) launches for all n frames; n <= 65535.  With `out`, a uint8 [n, stride],
    the rows are written there, and input that needs a conversion to contiguous fp32 goes through it in chunks of frames under
    `cap` bytes (a frame's pyramid depends on that frame only)."""
    int_in(levels, 1, MAX_LEVELS, "levels")
    n, H, W, C = check_images(images).shape
    if out is None:
        out = workspace(_cabi.load().lp_prop_pyramid_ws_bytes(n, H, W, levels), images.device, "lp_prop_pyramid_ws_bytes").view(n, -1)
        parts = [(0, n)]
    else:
        direct = images.dtype == torch.float32 and images.is_contiguous()
        parts = chunks(n, 1 if direct else H * W * C * 4, cap)
    for s, k in parts:
        part = _as_f32c(images[s:s + k])
        d = _cabi.LpPropLumaDesc(k, H, W, C, levels, 0, part.data_ptr(), out[s:s + k].data_ptr())
        launch("lp_prop_luma", images.device, ctypes.byref(d))
    return out


def row_addresses(t, n, first=0):
    """The device addresses of the rows first .. first + n - 1 of the contiguous `t`: a host uint64 [n]."""
    return np.uint64(t.data_ptr()) + np.arange(first, first + n, dtype=np.uint64) * np.uint64(t.stride(0) * t.element_size())


class FieldWalk:
    """The coarse-to-fine walk of the block matcher for at most `m` <= LP_PROP_MAX_JOBS independent jobs at a time: per level,
    top level first, lp_prop_match_batch then lp_prop_fill_batch, each level's final field the parent of the level below.  It
    owns the per-level scratch of its `m` rows, the host tables (uint64 [m, 6] and [m, 3] of device addresses per level) and
    the match descriptors; `run` fills the columns that name the jobs and allocates nothing.  `level0=False`: the caller says
    where the level-0 final fields go on every run, and no scratch is held for them."""

    def __init__(self, m, H, W, levels, search, smooth, dev, level0=True):
        int_in(m, 1, MAX_JOBS, "the jobs of a walk")
        self.levels, self.dev = levels, dev
        self.grids = [_cabi.prop_grid(H, W, lv) for lv in range(levels)]
        self._keep = []                                                  # the device buffers behind the addresses

        def rows(shape):
            self._keep.append(torch.empty((m, *shape), dtype=torch.int32, device=dev))
            return row_addresses(self._keep[-1], m)
        self.t_match = [np.zeros((m, 6), dtype=np.uint64) for _ in range(levels)]
        self.t_fill = [np.zeros((m, 3), dtype=np.uint64) for _ in range(levels)]
        for lv, (gh, gw) in enumerate(self.grids):
            self.t_match[lv][:, 4] = self.t_fill[lv][:, 0] = rows((gh, gw, 2))
            self.t_match[lv][:, 5] = self.t_fill[lv][:, 1] = rows((gh, gw))
            if lv or level0:
                self.t_fill[lv][:, 2] = rows((gh, gw, 2))
            if lv:
                self.t_match[lv - 1][:, 3] = self.t_fill[lv][:, 2]       # the parent: the level above's final field
        self.field0 = self.t_fill[0][:, 2].copy()                        # where level 0 goes when `run` is not told
        self.desc = [_cabi.LpPropMatchBatchDesc(H, W, levels, lv, search, smooth, 0, 0, self.t_match[lv].ctypes.data)
                     for lv in range(levels)]

    def run(self, src, tgt, weight, out=None):
        """The level-0 final fields of n <= m jobs, given as uint64 [n] address columns: the source frame's luma pyramid, the
        target frame's, and the pyramid of the bits that weight the match.  They go to the addresses `out`, or to the walk's
        own rows, `field0[:n]`, which the next run overwrites.  2 levels launches."""
        n = len(src)
        for t in self.t_match:
            t[:n, 0], t[:n, 1], t[:n, 2] = src, tgt, weight
        self.t_fill[0][:n, 2] = self.field0[:n] if out is None else out
        for lv in range(self.levels - 1, -1, -1):
            self.desc[lv].jobs = n
            launch("lp_prop_match_batch", self.dev, ctypes.byref(self.desc[lv]))
            launch("lp_prop_fill_batch", self.dev, self.t_fill[lv].ctypes.data, n, *self.grids[lv])
