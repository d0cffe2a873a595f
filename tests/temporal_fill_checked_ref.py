"""numpy restatement of the checked video temporal fill, written from include/lanpaint_hip.h ("Checked temporal fill" in the
lp_tfill_* section): the forward pass of tests/temporal_fill_ref.py unchanged, and a backward pass in which the forward sample
and the backward sample of a masked pixel are two witnesses.  Where both exist their 8-bit lumas are compared per aligned 8 x 8
block with a forgiven bias; a block that disagrees is left to the sampler.  Nothing here looks at the kernels."""
import numpy as np

from tests import propagate_ref as ref
from tests import temporal_fill_ref as tref

NONE, DISPUTED = -1, -2
BLOCK, MIN_PIXELS, MAX_BIAS = ref.BLOCK, ref.MIN_PIXELS, 32


def sample_luma(values):
    """fp32 [..., C] samples -> int64 [...]: the propagate section's 8-bit luma code of each."""
    return ref.luma(np.asarray(values, dtype=np.float32)).astype(np.int64)


def block_stats(both, d, agree):
    """Stage 3 per aligned 8 x 8 block, cut at the plane's edges: (n, mu, R, flag) int64 [gh, gw]; mu and R are 0 where
    n < MIN_PIXELS."""
    H, W = both.shape
    gh, gw = ref.grid_of(H, W)
    n, mu, R, flag = (np.zeros((gh, gw), np.int64) for _ in range(4))
    for by in range(gh):
        for bx in range(gw):
            win = (slice(8 * by, min(8 * by + BLOCK, H)), slice(8 * bx, min(8 * bx + BLOCK, W)))
            m, dd = both[win], d[win].astype(np.int64)
            k = int(m.sum())
            n[by, bx] = k
            if k < MIN_PIXELS:
                continue
            D = int(dd[m].sum())
            mu[by, bx] = min(max((2 * D + k) // (2 * k), -MAX_BIAS), MAX_BIAS)      # // is the mathematical floor
            R[by, bx] = int(np.abs(dd[m] - mu[by, bx]).sum())
            flag[by, bx] = int(R[by, bx] > agree * k)
    return n, mu, R, flag


def per_pixel(blocks, H, W):
    """A block plane [gh, gw] as a pixel plane [H, W]."""
    return np.repeat(np.repeat(blocks, BLOCK, axis=0), BLOCK, axis=1)[:H, :W]


def pair(t, known_t, images, org, pos, filled_t, source_t, remaining_t, agree, stats=None):
    """Stages 2 to 4 of the backward step for frame t: `org`, `pos` are B, the backward carry's state of t (tref.carry);
    `filled_t`, `source_t` and `remaining_t` are the frame's planes after the forward pass and are not altered.  Returns the
    frame's (filled, source, remaining, witnesses); `stats`, a dict, receives n, mu, R, flag and the pixel classes."""
    H, W = known_t.shape
    masked = known_t == 0
    has_a, has_b = masked & (source_t >= 0), masked & (org >= 0)
    both = has_a & has_b
    S_B = np.zeros_like(filled_t)
    S_B[has_b] = tref.sample(images, org[has_b], pos[has_b][:, 0], pos[has_b][:, 1])
    d = np.where(both, sample_luma(S_B) - sample_luma(filled_t), 0)
    n, mu, R, flag = block_stats(both, d, agree)
    disputed = both & (per_pixel(flag, H, W) == 1)
    enough = per_pixel(n, H, W) >= MIN_PIXELS
    write = tref.choose(t, known_t, org, np.where(source_t >= 0, source_t, NONE), True) & ~disputed
    filled, source, remaining = filled_t.copy(), source_t.astype(np.int64), remaining_t.copy()
    filled[write] = S_B[write]
    source[write] = org[write]
    remaining[write] = 0
    filled[disputed] = images[t][disputed]
    source[disputed] = DISPUTED
    remaining[disputed] = 1
    remaining[masked & ~has_a & ~has_b] = 1
    witnesses = np.where(disputed, 0, np.where(both & enough, 2, (has_a | has_b).astype(np.int64)))
    if stats is not None:
        stats.update(n=n, mu=mu, R=R, flag=flag, both=both, only_a=has_a & ~has_b, only_b=has_b & ~has_a,
                     neither=masked & ~has_a & ~has_b, disputed=disputed, d=d)
    return filled, source.astype(np.int32), remaining, witnesses.astype(np.int32)


def temporal_fill_checked_ref(images, mask, levels=4, search=2, smooth=8, reach=0, agree=8, trace=None):
    """The whole call: (filled fp32 [F, H, W, C], remaining fp32 [F, H, W], source int32 [F, H, W], witnesses int32 [F, H, W]).
    `trace`, a dict, receives per backward frame t the step's stats."""
    images = np.asarray(images, dtype=np.float32)
    F, H, W = images.shape[:3]
    known = tref.known_bits(np.asarray(mask, dtype=np.float32), F)
    Y = ref.luma(images)
    pyr = [ref.pyramid(Y[f], levels, ref.down_luma) for f in range(F)]
    kpyr = tref.known_pyramids(known, levels)
    source = np.where(known != 0, np.arange(F)[:, None, None], NONE).astype(np.int32)
    remaining = (known == 0).astype(np.float32)
    filled = images.copy()
    witnesses = np.zeros((F, H, W), np.int32)
    state = None
    for t in range(1, F):                                               # the forward pass: stages 3 and 4 with nearer = 0
        vec = tref.step_field(pyr[t], pyr[t - 1], kpyr[t], search, smooth)
        state = org, pos = tref.carry(t, known[t], t - 1, known[t - 1], vec, state, reach)
        write = tref.choose(t, known[t], org, source[t], False)
        filled[t][write] = tref.sample(images, org[write], pos[write][:, 0], pos[write][:, 1])
        source[t][write] = org[write]
        remaining[t][write] = 0
    witnesses[F - 1] = (known[F - 1] == 0) & (source[F - 1] >= 0)       # no backward step: A alone counts
    state = None
    for t in range(F - 2, -1, -1):
        vec = tref.step_field(pyr[t], pyr[t + 1], kpyr[t], search, smooth)
        state = org, pos = tref.carry(t, known[t], t + 1, known[t + 1], vec, state, reach)
        stats = {} if trace is not None else None
        filled[t], source[t], remaining[t], witnesses[t] = pair(t, known[t], images, org, pos, filled[t], source[t], remaining[t],
                                                                agree, stats)
        if trace is not None:
            trace[t] = stats
    return filled, remaining, source, witnesses
