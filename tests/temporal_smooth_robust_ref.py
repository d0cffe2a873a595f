"""numpy restatement of the robust video temporal smooth rule, written from include/lanpaint_hip.h (lp_tsmooth_robust): every masked
pixel walks along the motion into the past and the future, a chain ending only at the clip's end or the plane's edge; the lower
median of the samples' lumas names the reference r; what agrees with r is averaged, about the pixel where the pixel agrees too,
about r where two witnesses overrule it.  The fields, the codes and the sample are the plain restatement's
(tests/temporal_smooth_ref.py, tests/temporal_fill_ref.py, tests/propagate_ref.py).  Nothing here looks at the kernels."""
import numpy as np

from tests import propagate_ref as ref
from tests import temporal_fill_ref as tref
from tests import temporal_smooth_ref as sref

QUORUM = 2
MOTIONS = sref.MOTIONS


def luma_of(s):
    """fp32 [..., C] -> int64 [...]: the 8-bit luma of the codes; the first channel's code with fewer than three channels."""
    c = ref.codes(s)
    return (77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8 if c.shape[-1] >= 3 else c[..., 0]


def median_index(lumas, orders):
    """The rule's j* for one pixel: `lumas` and `orders` list Y_o and o of the existing samples, the own pixel (o = 0) among them.
    Fewer than three: 0.  Else the element at position (n - 1) >> 1 of the list sorted by (Y_o, o)."""
    n = len(orders)
    if n < 3:
        return 0
    return sorted(zip(lumas, orders))[(n - 1) >> 1][1]


def walk(images, known, fwd, bwd, radius, t, vectors=None):
    """The samples of the masked pixels of frame t: (ys, xs, exists bool [n, 2R + 1], s fp32 [n, 2R + 1, C]) by order index o;
    o = 0 is the own pixel.  `vectors`: a dict that keeps the per-pixel vectors of a field from frame to frame."""
    F, H, W, C = images.shape
    vectors = {} if vectors is None else vectors
    ys, xs = np.nonzero(known[t] == 0)
    n = len(ys)
    exists = np.zeros((n, 2 * radius + 1), bool)
    s = np.zeros((n, 2 * radius + 1, C), np.float32)
    exists[:, 0], s[:, 0] = True, images[t, ys, xs]
    for d, o0 in ((-1, 0), (1, radius)):
        alive = np.ones(n, bool)
        p = np.stack([16 * ys, 16 * xs], axis=-1).astype(np.int64)
        for k in range(1, radius + 1):
            u, v = t + (k - 1) * d, t + k * d
            if v < 0 or v >= F:
                break
            if (u, d) not in vectors:
                vectors[(u, d)] = ref.pixel_vectors((fwd if d == 1 else bwd)[u], H, W)
            i = (p + 8) >> 4
            q = p + vectors[(u, d)][np.clip(i[:, 0], 0, H - 1), np.clip(i[:, 1], 0, W - 1)]
            alive &= (q[:, 0] >= 0) & (q[:, 0] <= 16 * (H - 1)) & (q[:, 1] >= 0) & (q[:, 1] <= 16 * (W - 1))
            exists[:, o0 + k] = alive
            s[:, o0 + k] = tref.sample(images, np.full(n, v), q[:, 0], q[:, 1])   # of an ended chain: computed, never used
            p = np.where(alive[:, None], q, p)
    return ys, xs, exists, s


def reference_index(exists, s):
    """j* per pixel, int64 [n]: the lower median by (Y_o, o) of what exists."""
    n, slots = exists.shape
    key = luma_of(s) * 32 + np.arange(slots)[None, :]                     # (Y_o, o) as one number: o < 32
    key = np.where(exists, key, 1 << 20)                                 # what does not exist sorts behind everything
    count = exists.sum(axis=1)
    order = np.argsort(key, axis=1, kind="stable")
    js = order[np.arange(n), (np.maximum(count, 1) - 1) >> 1]
    return np.where(count < 3, 0, js).astype(np.int64)


def robust_frames(images, known, fwd, bwd, radius, tolerance, frames=None, trace=None):
    """The rule for the frames `frames` (all by default): (out fp32 [F, H, W, C], support int32 [F, H, W], replaced int32
    [F, H, W]); frames not asked for keep the images and -1 in both planes.  `trace` (a dict) receives what the tests ask about:
    per frame t the arrays (ys, xs, exists, j*, accepted, case)."""
    images = np.asarray(images, dtype=np.float32)
    F, H, W, C = images.shape
    w = sref.weights(radius)
    w_of = np.array([w[0]] + w[1:] + w[1:], np.int64)                    # by order index
    out = images.copy()
    support, replaced = np.full((F, H, W), -1, np.int32), np.full((F, H, W), -1, np.int32)
    vectors = {}
    for t in (range(F) if frames is None else frames):
        ys, xs, exists, s = walk(images, known, fwd, bwd, radius, t, vectors)
        n = len(ys)
        if n == 0:
            continue
        x = s[:, 0]
        js = reference_index(exists, s)
        r = s[np.arange(n), js]
        cr = ref.codes(r)
        accepted = exists & (np.abs(ref.codes(s) - cr[:, None, :]).max(axis=2) <= tolerance)
        own_ok = accepted[:, 0]
        a = accepted[:, 1:].sum(axis=1)
        base = np.where(own_ok[:, None], x, r).astype(np.float32)
        acc = np.zeros((n, C), np.float32)
        total = np.where(own_ok, w[0], 0).astype(np.int64)
        for o in range(1, 2 * radius + 1):                                # the walk's order: past 1..R, then future 1..R
            ok = accepted[:, o]
            total += np.where(ok, w_of[o], 0)
            ok = ok & (own_ok | (js != o))                                # r itself adds nothing where it is the base
            with np.errstate(invalid="ignore", over="ignore"):
                term = (np.float32(w_of[o]) * (s[:, o] - base).astype(np.float32)).astype(np.float32)
                acc = np.where(ok[:, None], (acc + term).astype(np.float32), acc)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            new = (base + (acc / total.astype(np.float32)[:, None]).astype(np.float32)).astype(np.float32)
        case = np.where(own_ok, 1, np.where(a >= QUORUM, 2, 3))
        moved = ((case == 1) & (a > 0)) | (case == 2)
        out[t, ys, xs] = np.where(moved[:, None], new, x)
        support[t, ys, xs] = np.where(case == 3, 0, a)
        replaced[t, ys, xs] = case == 2
        if trace is not None:
            trace[t] = (ys, xs, exists, js, accepted, case)
    return out, support, replaced


def temporal_smooth_robust_ref(images, mask, radius=2, tolerance=24, motion="background", levels=4, search=2, smooth=8, trace=None):
    """The whole call: (out fp32 [F, H, W, C], support int32 [F, H, W], replaced int32 [F, H, W])."""
    assert motion in MOTIONS
    images = np.asarray(images, dtype=np.float32)
    known = tref.known_bits(np.asarray(mask, dtype=np.float32), images.shape[0])
    fwd, bwd = sref.fields(images, known, motion, levels, search, smooth)
    return robust_frames(images, known, fwd, bwd, radius, tolerance, trace=trace)


def branches(trace, radius, frames):
    """Which of the rule's branches a run on a clip of `frames` took, from its trace: a set of names."""
    seen = set()
    for t, (ys, xs, exists, js, accepted, case) in trace.items():
        seen |= {f"case {c}" for c in np.unique(case).tolist()}
        seen |= {"replaced" if c == 2 else "not replaced" for c in np.unique(case).tolist()}
        if ((js >= 1) & (js <= radius)).any():
            seen.add("j* in the past")
        if (js > radius).any():
            seen.add("j* in the future")
        if (exists.sum(axis=1) < 3).any():
            seen.add("n < 3")
        for o0, room in ((0, min(radius, t)), (radius, min(radius, frames - 1 - t))):   # a direction: the steps the clip has room for
            e, ok = exists[:, o0 + 1:o0 + radius + 1], accepted[:, o0 + 1:o0 + radius + 1]
            behind = ok & (np.cumsum(e & ~ok, axis=1) > 0)              # accepted, with a rejected sample in front of it
            if (behind.any(axis=1) & (e.sum(axis=1) < room)).any():     # and the chain left the plane before the clip ended
                seen.add("a chain cut by the border with an accepted sample behind a rejected one")
    return seen


ALL_BRANCHES = {"case 1", "case 2", "case 3", "replaced", "not replaced", "j* in the past", "j* in the future", "n < 3",
                "a chain cut by the border with an accepted sample behind a rejected one"}
