"""Per-frame video masks from painted keyframes, built on the GPU.

Restates the reference's video mask pipeline (src/LanPaint/videomask.py, run by LanPaint_VideoMaskEditor,
nodes.py:890-995) with the per-pixel work in HIP (csrc/videomask_kernel.hip):

  1. every keyframe is binarised at 0.5 and gets an exact signed distance field (lp_vmask_edt, one job for all keyframes,
     which also returns exact integer centroid sums);
  2. the host turns the centroids into a per-frame plan -- zero / keyframe / inner frame with its blend weight and
     whole-pixel shifts -- in Python float arithmetic, which is the reference's own arithmetic (`frame_plan`);
  3. one launch morphs every frame (lp_vmask_morph) and, when the video size differs from the keyframes', writes the
     uint8 codes Pillow would be handed;
  4. one launch resizes them with Pillow's 8-bit BILINEAR from host-built coefficient tables (lp_vmask_resize).

The mask is made on the device and stays there.  HIP tensors only: there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import functools
import json
import math

import numpy as np
import torch

from . import _cabi
from ._hostcall import chunks, launch
from ._util import tables_for_launch

# one lp_vmask_frame of include/lanpaint_hip.h
FRAME_DTYPE = np.dtype([("kind", "<i4"), ("key_lo", "<i4"), ("key_hi", "<i4"), ("sx1", "<i4"), ("sy1", "<i4"),
                        ("sx2", "<i4"), ("sy2", "<i4"), ("reserved0", "<i4"), ("wf", "<f8"), ("omw", "<f8")])
_PRECISION_BITS = 22          # Pillow's fixed point for 8-bit images


def parse_keyframes_widget(value):
    """The editor's hidden `keyframes` widget, JSON {"<frame>": "<file>.png"}, as {frame: filename}.  Malformed JSON or a
    non-object gives {}; entries whose value is not a string or whose key is not an integer are dropped."""
    if not value:
        return {}
    try:
        data = json.loads(value)
    except (TypeError, ValueError):
        return {}
    if not isinstance(data, dict):
        return {}
    out = {}
    for key, name in data.items():
        if not isinstance(name, str):
            continue
        try:
            out[int(key)] = name
        except (TypeError, ValueError):
            continue
    return out


def load_keyframe_png(path):
    """A painted keyframe as float32 [h, w] in [0, 1]: the alpha channel when the image has one (the editor paints into
    alpha), otherwise its luminance.  Host-side PIL, imported on first use."""
    from PIL import Image
    with Image.open(path) as im:
        if "A" in im.getbands():
            band = im.getchannel("A")
        else:
            band = im if im.mode == "L" else im.convert("L")
        return np.asarray(band, dtype=np.float32) / 255.0


def audio_mask_frames(intervals, count, fps):
    """The editor's audio mask: [count] float32, 1 on the frames [max(0, floor(start*fps)), min(count, ceil(end*fps))) of
    every {start, end} interval (seconds) with end > start.  `intervals` is the widget's JSON string or the parsed list;
    malformed entries are skipped."""
    out = torch.zeros(count, dtype=torch.float32)
    if isinstance(intervals, str):
        try:
            intervals = json.loads(intervals)
        except (TypeError, ValueError):
            return out
    if not isinstance(intervals, list):
        return out
    for it in intervals:
        try:
            start, end = float(it.get("start", 0.0)), float(it.get("end", 0.0))
        except (AttributeError, TypeError, ValueError):
            continue
        if end > start:
            f0 = max(0, int(math.floor(start * fps)))
            f1 = min(count, int(math.ceil(end * fps)))
            if f1 > f0:
                out[f0:f1] = 1.0
    return out


def tap_window(center, support, in_size):
    """(first tap, tap count) of a filter of half-width `support` centred at `center` (source-pixel units), clipped to
    [0, in_size): Pillow's precompute_coeffs, which torch's antialiased interpolate took over (detail.aa_coeffs)."""
    xmin = max(int(center - support + 0.5), 0)
    return xmin, min(int(center + support + 0.5), in_size) - xmin


@functools.lru_cache(maxsize=64)
def pillow_bilinear_coeffs(in_size, out_size):
    """Pillow's BILINEAR coefficients for one axis (Resample.c precompute_coeffs + normalize_coeffs_8bpc, whole-image box):
    bounds int32 [out_size, 2] = (first source index, tap count), weights int32 [out_size, ksize] in 22-bit fixed point.
    Every quantity is a C double there and a Python float here, evaluated in the same order.  Cached (a few ms of Python
    per 1000 outputs); the arrays are read-only."""
    in_size, out_size = int(in_size), int(out_size)
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale                      # the bilinear filter's support is 1
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((out_size, 2), np.int32)
    weights = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin, xmax = tap_window(center, support, in_size)
        taps, ww = [], 0.0
        for x in range(xmax):
            w = abs((x + xmin - center + 0.5) * ss)
            w = 1.0 - w if w < 1.0 else 0.0
            taps.append(w)
            ww += w
        for x, w in enumerate(taps):
            if ww != 0.0:
                w /= ww
            weights[xx, x] = int(w * (1 << _PRECISION_BITS) + (-0.5 if w < 0 else 0.5))
        bounds[xx] = (xmin, xmax)
    bounds.flags.writeable = weights.flags.writeable = False
    return bounds, weights


def frame_plan(indices, count, centroids):
    """The per-frame table of lp_vmask_morph (FRAME_DTYPE [count]) for the sorted keyframe frame numbers `indices`;
    `centroids[j]` is keyframe j's foreground centroid (y, x), or None when it is empty.  Keyframe j is entry j of the key
    stack.  Frames before the first keyframe or after the last are zero; keyframes at or beyond `count` still bound the
    frames below `count` that lie before them."""
    plan = np.zeros(count, FRAME_DTYPE)
    if not any(i < count for i in indices):
        return plan
    for j, t in enumerate(indices):
        if t < count:
            plan[t]["kind"], plan[t]["key_lo"] = _cabi.LP_VMASK_KEY, j
    for j, (lo, hi) in enumerate(zip(indices, indices[1:])):
        c_lo, c_hi = centroids[j], centroids[j + 1]
        if c_lo is None or c_hi is None:
            dx, dy = 0.0, 0.0
        else:
            dx, dy = c_hi[1] - c_lo[1], c_hi[0] - c_lo[0]
        for t in range(lo + 1, min(hi, count)):
            wf = (t - lo) / (hi - lo)
            plan[t] = (_cabi.LP_VMASK_INNER, j, j + 1, math.floor(wf * dx + 0.5), math.floor(wf * dy + 0.5),
                       math.floor((1.0 - wf) * dx + 0.5), math.floor((1.0 - wf) * dy + 0.5), 0, wf, 1.0 - wf)
    return plan


def _device(device):
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("lanpaint_amd.videomask runs on a HIP device only; no CPU fallback")
        return torch.device("cuda", torch.cuda.current_device())
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"lanpaint_amd.videomask runs on a HIP device only; no CPU fallback (got {dev})")
    return dev


def _check_side(*sides):
    for s in sides:
        if not 0 < s <= _cabi.LP_VMASK_MAX_SIDE:
            raise ValueError(f"mask sides must lie in [1, {_cabi.LP_VMASK_MAX_SIDE}], got {s}")


def keyframe_edt(keys):
    """lp_vmask_edt on a float32 HIP tensor [K, h, w]: (d2 int32 [K, 2, h, w] -- squared distance to the nearest
    foreground / background pixel, LP_VMASK_D2_NONE where there is none --, sdf float64 [K, h, w], csum int64 [K, 3] =
    foreground count, sum of rows, sum of columns)."""
    keys = keys.to(torch.float32).contiguous()
    k, h, w = keys.shape
    _check_side(h, w)
    dev = keys.device
    d2 = torch.empty((k, 2, h, w), dtype=torch.int32, device=dev)
    sdf = torch.empty((k, h, w), dtype=torch.float64, device=dev)
    csum = torch.empty((k, 3), dtype=torch.int64, device=dev)
    d = _cabi.LpVmaskEdtDesc(k, h, w, 0, keys.data_ptr(), d2.data_ptr(), sdf.data_ptr(), csum.data_ptr())
    launch("lp_vmask_edt", dev, ctypes.byref(d))
    return d2, sdf, csum


EDT_BYTES_PER_PIXEL = 16              # what keyframe_edt allocates: two int32 planes and one fp64 per pixel


def edt_chunks(mask, cap_bytes):
    """keyframe_edt over the frames of a float32 HIP tensor [F, h, w], as many at a time as keep its buffers under `cap_bytes`
    (at least one): yields (start, count, d2 of those frames).  Frames are independent, so chunking cannot change a bit."""
    k, h, w = mask.shape
    _check_side(h, w)
    for s, n in chunks(k, EDT_BYTES_PER_PIXEL * h * w, cap_bytes):
        yield s, n, keyframe_edt(mask[s:s + n])[0]


def morph_frames(keys, plan, sdf=None, codes=False):
    """lp_vmask_morph: float32 [F, h, w] (or the uint8 codes trunc(m * 255) with `codes`) from the key stack [K, h, w],
    a FRAME_DTYPE plan [F] and the keyframes' SDF (None when the plan has no inner frame)."""
    keys = keys.to(torch.float32).contiguous()
    k, h, w = keys.shape
    dev = keys.device
    n = len(plan)
    table = torch.from_numpy(np.ascontiguousarray(plan).view(np.uint8).copy()).to(dev)
    out = torch.empty((n, h, w), dtype=torch.uint8 if codes else torch.float32, device=dev)
    if sdf is not None:
        sdf = sdf.contiguous()
        assert sdf.dtype == torch.float64 and tuple(sdf.shape) == (k, h, w)
    d = _cabi.LpVmaskMorphDesc(n, k, h, w, _cabi.LP_VMASK_OUT_U8 if codes else 0, 0, table.data_ptr(), keys.data_ptr(),
                               sdf.data_ptr() if sdf is not None else None, out.data_ptr())
    launch("lp_vmask_morph", dev, ctypes.byref(d))
    return out


def resize_codes(codes, size):
    """lp_vmask_resize: uint8 frames [F, h, w] on a HIP device to float32 [F, H, W] (size = (W, H)) as
    Image.fromarray(frame).resize(size, BILINEAR) / 255 does, frame by frame."""
    codes = codes.contiguous()
    if codes.dtype != torch.uint8 or codes.ndim != 3:
        raise ValueError("resize_codes takes uint8 frames [F, h, w]")
    n, h, w = codes.shape
    out_w, out_h = int(size[0]), int(size[1])
    _check_side(h, w, out_h, out_w)
    dev = codes.device
    bx, kx = tables_for_launch(pillow_bilinear_coeffs, dev, w, out_w)
    by, ky = tables_for_launch(pillow_bilinear_coeffs, dev, h, out_h)
    out = torch.empty((n, out_h, out_w), dtype=torch.float32, device=dev)
    d = _cabi.LpVmaskResizeDesc(n, h, w, out_h, out_w, kx.shape[1], ky.shape[1], 0, codes.data_ptr(),
                                bx.data_ptr(), kx.data_ptr(), by.data_ptr(), ky.data_ptr(), out.data_ptr())
    launch("lp_vmask_resize", dev, ctypes.byref(d))
    return out


def interpolate_masks(keyframes, count, size=None, device=None):
    """{frame: [h, w] mask in [0, 1]} (numpy arrays or tensors) -> float32 [count, H, W] on the HIP device: keyframes
    keep their painted values, frames between two keyframes get the SDF morph, frames outside the keyframe window are 0;
    then, when `size` = (W, H) differs from (w, h), Pillow's 8-bit BILINEAR up to it.  Unlike the reference, which raises
    IndexError when a frame between two keyframes lies at or beyond `count`, the frames 0..count-1 are returned.  With more
    than one keyframe the centroid sums [K, 3] are read back for the plan: the call's one device -> host read; with one
    keyframe there is none."""
    count = int(count)
    if count <= 0:
        raise ValueError("count must be positive")
    if not keyframes:
        raise ValueError("at least one keyframe is required")
    indices = sorted(keyframes)
    keys = [torch.as_tensor(np.asarray(v, dtype=np.float32)) if not torch.is_tensor(v) else v for v in
            (keyframes[i] for i in indices)]
    shapes = {tuple(v.shape) for v in keys}
    if len(shapes) != 1 or len(next(iter(shapes))) != 2:
        raise ValueError(f"every keyframe must be one [h, w] mask of the same size, got shapes {sorted(shapes)}")
    h, w = next(iter(shapes))
    out_w, out_h = (w, h) if size is None else (int(size[0]), int(size[1]))
    _check_side(h, w, out_h, out_w)
    resize = (out_w, out_h) != (w, h)
    dev = _device(device)
    if not any(i < count for i in indices):
        return torch.zeros((count, out_h, out_w), dtype=torch.float32, device=dev)
    stack = torch.stack([v.to(device=dev, dtype=torch.float32) for v in keys]).contiguous()
    centroids, sdf = [None] * len(indices), None
    if len(indices) > 1:
        _, sdf, csum = keyframe_edt(stack)
        centroids = [(sy / n, sx / n) if n else None for n, sy, sx in csum.cpu().tolist()]
    plan = frame_plan(indices, count, centroids)
    frames = morph_frames(stack, plan, sdf, codes=resize)
    return resize_codes(frames, (out_w, out_h)) if resize else frames
