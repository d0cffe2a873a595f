"""Shared arbiters of the video mask tests (tests/test_videomask_host.py, tests/test_gpu_videomask_shapes.py): the signed
distance field, the whole-pixel shift, the SDF morph and its uint8 codes restated in float64 numpy from the formula in
lanpaint_amd/videomask.py, and live Pillow for the resize.  Nothing here touches a device.

    m(t) = float32(1 / (1 + exp(-clip(omw * S(sdf_lo, sy1, sx1) + wf * S(sdf_hi, -sy2, -sx2), -50, 50))))
    S(f, dy, dx)(y, x) = f(y - dy, x - dx), 0 outside;  sdf = edt(fg) - edt(~fg), fg = key >= 0.5
"""
import numpy as np

from lanpaint_amd import _cabi

try:
    from scipy import ndimage as _ndimage
except ImportError:                                        # the numpy EDT below then stands alone
    _ndimage = None


def edt_numpy(a):
    """float64 distance of every True pixel of `a` to its nearest False pixel (0 on False pixels), by exact integer
    arithmetic: the distance to the nearest False pixel of the own column, then per row the minimum over the columns u of
    g(u)^2 + (x - u)^2.  O(h * w * w): for fixture-sized masks.  `a` must hold a False pixel."""
    a = np.asarray(a, bool)
    h, w = a.shape
    assert not a.all(), "no False pixel to measure to"
    rows = np.arange(h, dtype=np.int64)[:, None]
    far = np.int64(4 * (h + w))                            # further than any pixel of the frame
    above = np.maximum.accumulate(np.where(a, -far, rows), 0)            # nearest False row at or above
    below = np.minimum.accumulate(np.where(a, far, rows)[::-1], 0)[::-1]  # ... at or below
    g = np.minimum(rows - above, below - rows)
    g2 = np.where(g >= far - h, np.int64(1) << 60, g * g)  # a column without a False pixel never wins
    xs = np.arange(w, dtype=np.int64)[None, :]
    d2 = np.full((h, w), np.iinfo(np.int64).max, np.int64)
    for u in range(w):
        np.minimum(d2, g2[:, u:u + 1] + (xs - u) ** 2, out=d2)
    return np.sqrt(d2.astype(np.float64))


def edt(a):
    """scipy.ndimage.distance_transform_edt when scipy is importable, else `edt_numpy` (they agree exactly)."""
    if _ndimage is not None:
        return _ndimage.distance_transform_edt(np.asarray(a, bool))
    return edt_numpy(a)


def sdf_ref(key):
    """float64 [h, w]: distance to the background minus distance to the foreground of `key >= 0.5`; an empty key is
    -max(h, w) / 2 everywhere, a full one +max(h, w) / 2."""
    fg = np.asarray(key) >= 0.5
    h, w = fg.shape
    if not fg.any():
        return np.full((h, w), -max(h, w) / 2.0, np.float64)
    if fg.all():
        return np.full((h, w), max(h, w) / 2.0, np.float64)
    return edt(fg) - edt(~fg)


def shift_ref(field, dy, dx):
    """out[y, x] = field[y - dy, x - dx], 0 where that lies outside the frame; any integers dy, dx."""
    field = np.asarray(field)
    h, w = field.shape
    dy, dx = int(dy), int(dx)
    out = np.zeros_like(field)
    y0, y1 = max(0, dy), min(h, h + dy)                    # the destination rows that have a source row
    x0, x1 = max(0, dx), min(w, w + dx)
    if y1 > y0 and x1 > x0:
        out[y0:y1, x0:x1] = field[y0 - dy:y1 - dy, x0 - dx:x1 - dx]
    return out


def morph_ref(keys, plan):
    """float32 [F, h, w] for a FRAME_DTYPE plan over the key stack [K, h, w]: ZERO frames are 0, KEY frames the key's painted
    values, INNER frames the sigmoid of the blended, shifted SDFs -- evaluated in float64, each product and the sum rounded
    on its own -- and an entry whose key index lies outside [0, K) is 0."""
    keys = np.asarray(keys, np.float32)
    n_keys, h, w = keys.shape
    sdfs = {}

    def sdf(j):
        if j not in sdfs:
            sdfs[j] = sdf_ref(keys[j])
        return sdfs[j]

    out = np.zeros((len(plan), h, w), np.float32)
    for t, p in enumerate(plan):
        lo, hi = int(p["key_lo"]), int(p["key_hi"])
        if p["kind"] == _cabi.LP_VMASK_KEY and 0 <= lo < n_keys:
            out[t] = keys[lo]
        elif p["kind"] == _cabi.LP_VMASK_INNER and 0 <= lo < n_keys and 0 <= hi < n_keys:
            a = np.float64(p["omw"]) * shift_ref(sdf(lo), p["sy1"], p["sx1"])
            b = np.float64(p["wf"]) * shift_ref(sdf(hi), -int(p["sy2"]), -int(p["sx2"]))
            v = np.clip(a + b, -50.0, 50.0)
            out[t] = (1.0 / (1.0 + np.exp(-v))).astype(np.float32)
    return out


def codes_ref(m32):
    """The uint8 codes the resize is handed: the fp32 product truncated."""
    m32 = np.asarray(m32)
    assert m32.dtype == np.float32
    return (m32 * np.float32(255)).astype(np.uint8)


def pil_resize_ref(codes, size):
    """uint8 frames [F, h, w] -> float32 [F, H, W], size = (W, H): live Pillow's BILINEAR, frame by frame, over 255."""
    from PIL import Image
    codes = np.asarray(codes)
    assert codes.dtype == np.uint8 and codes.ndim == 3
    size = (int(size[0]), int(size[1]))
    return np.stack([np.asarray(Image.fromarray(f).resize(size, Image.BILINEAR), np.float32) / np.float32(255)
                     for f in codes])


def ulp_diff(a, b):
    """|a - b| in units of fp32 spacing, elementwise, for finite non-negative fp32 arrays (bit patterns are then ordered)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
