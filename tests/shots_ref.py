"""numpy restatement of the video shot detect rule, written from include/lanpaint_hip.h (lp_shot_*): the two integer scores of
every pair of neighbouring frames, the decision and the shot index.  The planes are the propagate restatement's luma pyramids.
Nothing here looks at the kernels."""
import numpy as np

from tests import propagate_ref as ref

BLOCK, BINS = ref.BLOCK, 64
MAX_LEVEL, MAX_SEARCH, MAX_WINDOW = 5, 3, 16


def planes(images, level=2):
    """fp32 [F, H, W, C] -> uint8 [F, h, w]: level `level` of every frame's luma pyramid."""
    return ref.pyramid(ref.luma(images), level + 1, ref.down_luma)[level]


def residual(Ya, Yb, search):
    """A of the pair (Ya, Yb): per 8 x 8 block cut at the plane's edges the least SAD over the displacements, summed."""
    h, w = Ya.shape
    a = Ya.astype(np.int64)
    b = Yb.astype(np.int64)
    ys, xs = np.arange(h), np.arange(w)
    sads = []
    for dy in range(-search, search + 1):
        for dx in range(-search, search + 1):
            moved = b[np.clip(ys + dy, 0, h - 1)][:, np.clip(xs + dx, 0, w - 1)]
            diff = np.abs(a - moved)
            rows = np.add.reduceat(diff, np.arange(0, h, BLOCK), axis=0)
            sads.append(np.add.reduceat(rows, np.arange(0, w, BLOCK), axis=1))
    return int(np.min(np.stack(sads), axis=0).sum())


def histogram(Y):
    return np.bincount((Y.astype(np.int64) >> 2).ravel(), minlength=BINS)


def scores_of_planes(Y, search=2):
    """uint8 [F, h, w] -> int64 [F - 1, 2]: (A, B) per pair."""
    if not 1 <= search <= MAX_SEARCH:
        raise ValueError("search")
    hist = [histogram(y) for y in Y]
    out = np.zeros((len(Y) - 1, 2), np.int64)
    for t in range(len(Y) - 1):
        out[t] = residual(Y[t], Y[t + 1], search), int(np.abs(hist[t] - hist[t + 1]).sum())
    return out


def shot_scores(images, level=2, search=2):
    """(score int64 [F - 1, 2], N)."""
    if not 0 <= level <= MAX_LEVEL:
        raise ValueError("level")
    Y = planes(images, level)
    return scores_of_planes(Y, search), int(Y.shape[1] * Y.shape[2])


def cuts(score, n_pixels, threshold, hist, ratio=200, window=4):
    """uint8 [F - 1]: the three conditions, in int64 (every product stays below 2^50)."""
    if not (1 <= threshold <= 255 and 0 <= hist <= 100 and 100 <= ratio <= 10000 and 1 <= window <= MAX_WINDOW and n_pixels >= 1):
        raise ValueError("a parameter outside its range")
    score = np.asarray(score, dtype=np.int64).reshape(-1, 2)
    A, B = score[:, 0], score[:, 1]
    ok = (A >= threshold * n_pixels) & (100 * B >= hist * 2 * n_pixels)
    for k in range(1, min(window, len(A) - 1) + 1):                    # the pairs k in front of t, and k behind it
        ok[k:] &= 100 * A[k:] >= ratio * A[:-k]
        ok[:-k] &= 100 * A[:-k] >= ratio * A[k:]
    return ok.astype(np.uint8)


def shot_decide(score, n_pixels, threshold, hist, ratio=200, window=4):
    """int32 [F]: shot[0] = 0, shot[f] = the cuts in front of f."""
    c = cuts(score, n_pixels, threshold, hist, ratio, window)
    return np.concatenate([[0], np.cumsum(c.astype(np.int64))]).astype(np.int32)


def detect_shots(images, threshold, hist, ratio=200, window=4, level=2, search=2):
    score, n = shot_scores(images, level, search)
    return shot_decide(score, n, threshold, hist, ratio, window), score


def shot_ranges(shot):
    """[(lo, hi), ...]: the frames of every shot."""
    shot = [int(v) for v in np.asarray(shot)]
    edges = [0] + [f for f in range(1, len(shot)) if shot[f] != shot[f - 1]] + [len(shot)]
    return list(zip(edges[:-1], edges[1:]))
