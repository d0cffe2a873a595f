"""The patch form of lp_mask_fill restated in numpy from the rule's text (include/lanpaint_hip.h, LP_FILL_PATCH): whole-level array
operations over all targets at once -- a search round reads one field and writes another, so it has no order between pixels --
no tiles, no LDS, no early exit.  The pre-fill is tests/fill_ref.py's, the Philox block tests/grain_ref.py's."""
import numpy as np

from tests import fill_ref
from tests.grain_ref import philox4x32_10

INVALID = -1
BIG = np.int64(1) << 40                                             # above every distance: 81 * 4 * 255
MAX_RADIUS, MAX_LEVELS, MAX_ITERS, MAX_CHANNELS = 4, 6, 8, 4


def mode_word(r, levels, iters, seed):
    """LP_FILL_PATCH as an int32."""
    word = 1 | (r << 4) | (levels << 8) | (iters << 12) | (seed << 16)
    return word - (1 << 32) if word >= 1 << 31 else word


def auto_levels(h, w, r):
    """The wrapper's AUTO: the largest L in 1..6 with min(h_{L-1}, w_{L-1}) >= 4 (2 r + 1), at least 1."""
    best = 1
    for L in range(1, MAX_LEVELS + 1):
        if min(h, w) >= 4 * (2 * r + 1):
            best = L
        h, w = (h + 1) // 2, (w + 1) // 2
    return best


def codes_of(v):
    """clamp(floor(fl(fl(v * 255) + 0.5)), 0, 255) in fp32, a NaN gives 0: int64."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.floor(v.astype(np.float32) * np.float32(255) + np.float32(0.5))
    t = np.where(np.isnan(t), np.float32(0), t)
    return np.clip(t, 0, 255).astype(np.int64)


def down(I, hole):
    """One level up: I [h, w, C] int64, hole [h, w] bool -> the rounded mean of the children inside, the OR of their flags."""
    h, w, C = I.shape
    h2, w2 = (h + 1) // 2, (w + 1) // 2
    Ip, inside, hp = np.zeros((2 * h2, 2 * w2, C), np.int64), np.zeros((2 * h2, 2 * w2), np.int64), np.zeros((2 * h2, 2 * w2), bool)
    Ip[:h, :w], inside[:h, :w], hp[:h, :w] = I, 1, hole
    s = sum(Ip[dy::2, dx::2] for dy in (0, 1) for dx in (0, 1))
    n = sum(inside[dy::2, dx::2] for dy in (0, 1) for dx in (0, 1))[..., None]
    return (s + n // 2) // n, hp[0::2, 0::2] | hp[0::2, 1::2] | hp[1::2, 0::2] | hp[1::2, 1::2]


def sets_of(hole, r):
    """(target, source) of a level: the hole dilated by r inside the picture; whole patch inside and hole-free."""
    h, w = hole.shape
    hp = np.zeros((h + 2 * r, w + 2 * r), bool)
    hp[r:r + h, r:r + w] = hole
    near = np.zeros((h, w), bool)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            near |= hp[dy:dy + h, dx:dx + w]
    y, x = np.mgrid[0:h, 0:w]
    whole = (y - r >= 0) & (y + r < h) & (x - r >= 0) & (x + r < w)
    return near, whole & ~near


class Level:
    def __init__(self, I, hole, r):
        self.I, self.hole, self.r = I, hole, r
        self.h, self.w = hole.shape
        self.target, self.source = sets_of(hole, r)
        self.T = I.copy()
        self.py, self.px = np.nonzero(self.target)                      # the targets, raster order
        self.qy, self.qx = np.nonzero(hole)

    def distance(self, sy, sx, ok):
        """D(p, s) for every target p and its candidate s, where `ok`; BIG elsewhere."""
        r, h, w = self.r, self.h, self.w
        sy, sx = np.where(ok, sy, r), np.where(ok, sx, r)               # (any place whose patch can be read)
        Tp = np.zeros((h + 2 * r, w + 2 * r, self.T.shape[2]), np.int64)
        Tp[r:r + h, r:r + w] = self.T
        D = np.zeros(len(self.py), np.int64)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                ty, tx = self.py + dy, self.px + dx
                inside = (ty >= 0) & (ty < h) & (tx >= 0) & (tx < w)
                diff = np.abs(Tp[ty + r, tx + r] - self.I[np.clip(sy + dy, 0, h - 1), np.clip(sx + dx, 0, w - 1)]).sum(axis=1)
                D += np.where(inside, diff, 0)
        return np.where(ok, D, BIG)

    def search(self, nnf, level, rnd, seed):
        """One round: the field [h, w, 2] (INVALID: -1) -> the next one."""
        h, w, py, px = self.h, self.w, self.py, self.px
        best_d = np.full(len(py), BIG, np.int64)
        best_y, best_x = np.full(len(py), INVALID, np.int64), np.full(len(py), INVALID, np.int64)

        def consider(cy, cx, ok):
            nonlocal best_d, best_y, best_x
            ok = ok & (cy >= 0) & (cy < h) & (cx >= 0) & (cx < w)
            ok = ok & self.source[np.clip(cy, 0, h - 1), np.clip(cx, 0, w - 1)]
            D = self.distance(cy, cx, ok)
            better = ok & ((D < best_d) | ((D == best_d) & ((cy < best_y) | ((cy == best_y) & (cx < best_x)))))
            best_d, best_y, best_x = np.where(better, D, best_d), np.where(better, cy, best_y), np.where(better, cx, best_x)

        own = nnf[py, px]
        consider(own[:, 0], own[:, 1], own[:, 0] >= 0)
        for step in (1, 4):
            for ey, ex in ((0, -1), (-1, 0), (0, 1), (1, 0)):
                ny, nx = py + step * ey, px + step * ex
                inside = (ny >= 0) & (ny < h) & (nx >= 0) & (nx < w)
                cy_, cx_ = np.clip(ny, 0, h - 1), np.clip(nx, 0, w - 1)
                e = nnf[cy_, cx_]
                consider(e[:, 0] - step * ey, e[:, 1] - step * ex, inside & self.target[cy_, cx_] & (e[:, 0] >= 0))
        j = 0
        while (max(h, w) >> j) >= 1:
            R = max(h, w) >> j
            valid = best_y >= 0
            cy, cx = np.where(valid, best_y, py), np.where(valid, best_x, px)
            ctr = py.astype(np.uint64) * np.uint64(65536) + px.astype(np.uint64)
            sub = np.uint64((level << 40) | (rnd << 32) | j)
            w0, w1, _, _ = philox4x32_10(ctr, sub, np.uint64(seed))
            span = np.uint64(2 * R + 1)
            uy = ((w0 * span) >> np.uint64(32)).astype(np.int64) - R
            ux = ((w1 * span) >> np.uint64(32)).astype(np.int64) - R
            consider(cy + uy, cx + ux, np.ones(len(py), bool))
            j += 1
        out = np.full((h, w, 2), INVALID, np.int64)
        out[py, px, 0], out[py, px, 1] = best_y, best_x
        return out

    def vote(self, nnf):
        """T at the hole pixels from the field; -> voted [h, w] bool (n > 0)."""
        r, h, w, qy, qx = self.r, self.h, self.w, self.qy, self.qx
        s = np.zeros((len(qy), self.I.shape[2]), np.int64)
        n = np.zeros(len(qy), np.int64)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                y, x = qy - dy, qx - dx
                inside = (y >= 0) & (y < h) & (x >= 0) & (x < w)
                e = nnf[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)]
                ok = inside & (e[:, 0] >= 0)
                val = self.I[np.clip(e[:, 0] + dy, 0, h - 1), np.clip(e[:, 1] + dx, 0, w - 1)]
                s += np.where(ok[:, None], val, 0)
                n += ok
        got = n > 0
        nn = np.where(got, n, 1)[:, None]
        self.T[qy[got], qx[got]] = ((s + nn // 2) // nn)[got]
        voted = np.zeros((h, w), bool)
        voted[qy[got], qx[got]] = True
        return voted

    def field_from(self, coarse):
        """The level's first field from the one the level above ended with."""
        h, w = self.h, self.w
        out = np.full((h, w, 2), INVALID, np.int64)
        y, x = np.mgrid[0:h, 0:w]
        up = coarse[y >> 1, x >> 1]
        sy, sx = 2 * up[..., 0] + (y & 1), 2 * up[..., 1] + (x & 1)
        ok = self.target & (up[..., 0] >= 0) & (sy < h) & (sx < w)
        ok &= self.source[np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)]
        out[ok, 0], out[ok, 1] = sy[ok], sx[ok]
        return out


def fill_one(image, mask, r, levels, iters, seed):
    """image [H, W, C] fp32, C <= 4, mask [H, W] -> (out [H, W, C] fp32, the level-0 field as s_y * 65536 + s_x or -1 [H, W] int32,
    the level-0 targets [H, W] bool)."""
    pp = fill_ref.fill_one(image, mask)
    I, hole = codes_of(pp), mask > 0.5
    pyramid = [Level(I, hole, r)]
    for _ in range(1, levels):
        I, hole = down(I, hole)
        pyramid.append(Level(I, hole, r))
    nnf, voted = None, None
    for l in range(levels - 1, -1, -1):
        g = pyramid[l]
        if nnf is None:
            nnf = np.full((g.h, g.w, 2), INVALID, np.int64)
        else:
            nnf = g.field_from(nnf)
            g.vote(nnf)
        for rnd in range(iters):
            nnf = g.search(nnf, l, rnd, seed)
            voted = g.vote(nnf)
    g = pyramid[0]
    out = pp.copy()
    filled = (g.T.astype(np.float32) / np.float32(255.0)).astype(np.float32)
    out[voted] = filled[voted]
    known = ~(mask > 0.5)
    out[known] = image[known]
    field = np.where(nnf[..., 0] >= 0, nnf[..., 0] * 65536 + nnf[..., 1], INVALID).astype(np.int32)
    return out, field, g.target


def fill_ref_patch(image, mask, r, levels, iters, seed):
    """image [B, H, W, C] fp32, mask [Bm, H, W], Bm 1 or B -> (out [B, H, W, C], fields [B, H, W] int32, targets [B, H, W] bool)."""
    parts = [fill_one(image[b], mask[b % mask.shape[0]], r, levels, iters, seed) for b in range(image.shape[0])]
    return tuple(np.stack([p[i] for p in parts]) for i in range(3))
