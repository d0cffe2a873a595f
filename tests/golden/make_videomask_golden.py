#!/usr/bin/env python3
"""Record the UNMODIFIED reference's video masks (src/LanPaint/videomask.py: interpolate_masks + resize_masks, the path
LanPaint_VideoMaskEditor runs, nodes.py:890-995) into tests/golden/videomask_*.npz for tests/test_videomask_host.py and
tests/test_gpu_videomask.py:

    keys [K, h, w] float32, indices [K], count, size (W, H)
    frames       the frame numbers whose masks are stored below: every frame, except in the large case, which keeps a
                 fixed sample (keyframes, early / middle / late inner frames) so that the file stays small
    morph        the reference's masks of those frames before the resize, [len(frames), h, w] float32
                 (morph_codes: its uint8 codes trunc(m * 255) instead, for the large case)
    final_codes  the resized masks as uint8 codes (final = code / 255, what resize_masks returns), when size != (w, h)
    shifts       the whole-pixel shifts the reference applied, one row (sy1, sx1, -sy2, -sx2) per inner frame, in frame
                 order, and inner_frames, the frame numbers they belong to (recorded by wrapping its _shift)

Run where a checkout of the reference tree and scipy are at hand (the reference's exact EDT; without scipy it falls back to
a pure-Python one that gives the same distances, very slowly):
    python tests/golden/make_videomask_golden.py PATH_TO_REFERENCE
The reference module is loaded from its file under a private name; sys.path and sys.dont_write_bytecode are restored
afterwards.  Nothing of it is copied.
"""
from __future__ import annotations

import contextlib
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


@contextlib.contextmanager
def reference_videomask(ref_root):
    saved_path, saved_flag = list(sys.path), sys.dont_write_bytecode
    sys.dont_write_bytecode = True
    try:
        spec = importlib.util.spec_from_file_location("_lanpaint_reference_videomask",
                                                      os.path.join(ref_root, "src", "LanPaint", "videomask.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        yield mod
    finally:
        sys.path[:] = saved_path
        sys.dont_write_bytecode = saved_flag


def disk(h, w, cy, cx, r, soft=0.0):
    yy, xx = np.mgrid[:h, :w].astype(np.float64)
    d = np.sqrt((yy - cy) ** 2 + (xx - cx) ** 2) - r
    if soft <= 0:
        return (d <= 0).astype(np.float32)
    v = np.clip(0.5 - d / soft, 0.0, 1.0)
    return (np.round(v * 255.0) / 255.0).astype(np.float32)        # what a painted PNG's alpha gives


def cases():
    rng = np.random.default_rng(7)
    h, w = 40, 56
    empty, full = np.zeros((h, w), np.float32), np.ones((h, w), np.float32)
    blob = disk(h, w, 20, 30, 9) * (rng.random((h, w)) > 0.05)          # holes: a ragged foreground
    yield "translate", {0: disk(h, w, 12, 10, 6), 9: disk(h, w, 25, 44, 8)}, 12, (w, h)
    # D = (+45, +1): the shifted fields run mostly off the frame; vacated pixels read 0
    yield "translate_far", {0: disk(h, w, 20, 4, 5), 6: disk(h, w, 21, 49, 5)}, 7, (97, 61)
    yield "grow_shrink_full", {0: empty, 4: disk(h, w, 18, 25, 7), 8: empty, 12: full, 15: blob}, 16, (w, h)
    # non-adjacent and adjacent keyframes, soft values, the last keyframe exactly at count (an endpoint, no raise)
    soft = {1: disk(h, w, 10, 10, 6, 3.0), 2: disk(h, w, 11, 12, 6, 3.0), 3: disk(h, w, 30, 40, 4, 2.0),
            9: disk(h, w, 20, 28, 12, 4.0), 18: disk(h, w, 5, 50, 3, 1.5)}
    yield "multi_soft", soft, 18, (w, h)
    yield "multi_soft_down", soft, 18, (23, 17)
    yield "single", {3: disk(h, w, 20, 20, 10, 3.0)}, 6, (61, 97)
    yield "all_beyond", {7: disk(h, w, 20, 20, 10), 9: full}, 5, (33, 21)
    # keyframes {0, 9} with count 5: the reference raises IndexError; the expected frames are the first 5 of count 10
    yield "beyond_end", {0: disk(h, w, 10, 10, 5), 9: disk(h, w, 30, 45, 7)}, 5, (w, h)
    # D = (3, -3) at wf = 1/2: wf*dx + 0.5 = 2.0 and wf*dy + 0.5 = -1.0 exactly
    yield "exact_half", {0: disk(h, w, 20, 20, 6), 2: disk(h, w, 17, 23, 6)}, 3, (57, 41)
    yield "odd_sizes", {0: disk(31, 45, 9, 12, 7, 2.0), 4: disk(31, 45, 20, 30, 5, 2.0)}, 7, (19, 53)
    H, W = 480, 832
    yield "realistic", {0: disk(H, W, 200, 260, 90, 6.0), 80: disk(H, W, 290, 560, 120, 6.0)}, 81, (1280, 720)


# frames stored for the large case: the two keyframes and inner frames at both ends and in the middle of the morph
LARGE_FRAMES = (0, 1, 2, 39, 40, 41, 78, 79, 80)


def record(ref, name, keyframes, count, size):
    indices = sorted(keyframes)
    inner_pairs = [(lo, hi) for lo, hi in zip(indices, indices[1:]) if hi - lo > 1]
    ref_count = max([count] + [hi for lo, hi in inner_pairs if lo + 1 < count])   # where the reference would raise
    calls = []
    shift = ref._shift

    def recording_shift(field, dy, dx):
        calls.append((int(dy), int(dx)))
        return shift(field, dy, dx)
    ref._shift = recording_shift
    try:
        morph = ref.interpolate_masks(dict(keyframes), ref_count)[:count]
    finally:
        ref._shift = shift
    inner = [t for lo, hi in inner_pairs for t in range(lo + 1, hi)] if len(indices) > 1 and indices[0] < ref_count else []
    assert len(calls) == 2 * len(inner), (name, len(calls), len(inner))
    shifts = np.array([calls[2 * i] + calls[2 * i + 1] for i in range(len(inner))], np.int32).reshape(-1, 4)
    keep = np.array([t < count for t in inner], bool)
    h, w = morph.shape[1:]
    rec = dict(keys=np.stack([keyframes[i] for i in indices]).astype(np.float32), indices=np.array(indices, np.int64),
               count=np.int64(count), size=np.array(size, np.int64), shifts=shifts[keep] if len(inner) else shifts,
               inner_frames=np.array([t for t in inner if t < count], np.int64))
    large = morph.size > 4_000_000
    frames = np.array([t for t in LARGE_FRAMES if t < count] if large else range(count), np.int64)
    rec["frames"] = frames
    if large:
        rec["morph_codes"] = (morph[frames] * 255).astype(np.uint8)
    else:
        rec["morph"] = morph
    if tuple(size) != (w, h):
        final = ref.resize_masks(morph[frames], tuple(size))
        codes = np.round(final * 255.0).astype(np.uint8)
        assert np.array_equal(codes.astype(np.float32) / 255.0, final)
        rec["final_codes"] = codes
    path = os.path.join(HERE, f"videomask_{name}.npz")
    np.savez_compressed(path, **rec)
    return path


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "src", "LanPaint")):
        raise SystemExit("usage: make_videomask_golden.py PATH_TO_REFERENCE  (the directory holding src/LanPaint)")
    with reference_videomask(os.path.abspath(sys.argv[1])) as ref:
        if ref._scipy_edt is None:
            raise SystemExit("scipy is needed: the fixtures are recorded on the reference's scipy EDT path")
        total = 0
        for name, keyframes, count, size in cases():
            path = record(ref, name, keyframes, count, size)
            total += os.path.getsize(path)
            print(os.path.basename(path), os.path.getsize(path), "bytes")
        print("total", total, "bytes")


if __name__ == "__main__":
    main()
