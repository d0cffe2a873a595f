"""numpy restatement of the video temporal fill rule, written from include/lanpaint_hip.h (lp_tfill_*): what lies under the mask of
a frame is borrowed from the nearest frame in which the same piece of background is visible.  The motion of the known pixels is
the propagate section's block field (tests/propagate_ref.py), weighted by the mask's complement; an origin (frame, position) is
carried along it frame by frame, forwards and backwards, and the picture is sampled once at the origin.  Nothing here looks at
the kernels."""
import numpy as np

from tests import propagate_ref as ref

NONE = -1
WHOLE_CLIP = 1 << 30                  # reach 0: no age is too large


def known_bits(mask, frames):
    """mask [F, H, W], [1, H, W] or [H, W] -> uint8 [F, H, W]: 1 where the picture is known (mask < 0.5, or a NaN)."""
    m = ref.binarise(mask)
    if m.ndim == 2:
        m = m[None]
    if m.shape[0] == 1 and frames > 1:
        m = np.repeat(m, frames, axis=0)
    return (1 - m).astype(np.uint8)


def known_pyramids(known, levels):
    """Per frame the pyramid of its known bits: the OR over the footprints of the propagate section's stage 2."""
    return [ref.pyramid(k, levels, ref.down_mask) for k in known]


def step_field(pyr_t, pyr_donor, kpyr_t, search, smooth):
    """The level-0 final field of the step from frame t to its donor, weighted by t's known bits."""
    return ref.motion_field(pyr_t, pyr_donor, kpyr_t, search, smooth)[0]


def first_state(t, known_t):
    """The state of the first frame of a direction: only its known pixels have an origin, themselves."""
    H, W = known_t.shape
    return np.where(known_t != 0, t, NONE).astype(np.int64), ref.key_positions(H, W)


def carry(t, known_t, donor, known_donor, vec, state_donor, reach):
    """One step of one direction.  `state_donor` (org int64 [H, W], pos int64 [H, W, 2]) is read under the donor's mask only:
    under its known pixels the origin is (donor, (16 y, 16 x)).  None: the donor is the first frame of the direction.
    Returns t's (org, pos) with the known pixels filled in; pos is 0 where org is NONE."""
    H, W = known_t.shape
    own = ref.key_positions(H, W)
    if state_donor is None:
        state_donor = first_state(donor, known_donor)
    s_org = np.where(known_donor != 0, donor, state_donor[0]).astype(np.int64)
    s_pos = np.where((known_donor != 0)[..., None], own, state_donor[1]).astype(np.int64)
    V = ref.pixel_vectors(vec, H, W)
    q = own + V
    inside = (q[..., 0] >= 0) & (q[..., 0] <= 16 * (H - 1)) & (q[..., 1] >= 0) & (q[..., 1] <= 16 * (W - 1))
    i = (q + 8) >> 4
    r = q - 16 * i
    iy, ix = np.clip(i[..., 0], 0, H - 1), np.clip(i[..., 1], 0, W - 1)
    f = s_org[iy, ix]
    found = inside & (f >= 0) & (np.abs(t - f) <= (reach if reach else WHOLE_CLIP))
    P = s_pos[iy, ix] + r
    is_known = known_t != 0
    org = np.where(is_known, t, np.where(found, f, NONE)).astype(np.int64)
    pos = np.where(is_known[..., None], own, np.where(found[..., None], P, 0)).astype(np.int64)
    return org, pos


def sample(images, f, Py, Px):
    """images fp32 [F, H, W, C] at frames f and positions (Py, Px) in 1/16 px, clamped to the plane: fp32 [n, C].  Every
    product and sum is rounded to fp32 on its own; a tap with weight 0 is not read."""
    H, W = images.shape[1:3]
    Py, Px = np.clip(Py, 0, 16 * (H - 1)), np.clip(Px, 0, 16 * (W - 1))
    iy, ix, fy, fx = Py >> 4, Px >> 4, Py & 15, Px & 15
    iy1, ix1 = np.minimum(iy + 1, H - 1), np.minimum(ix + 1, W - 1)
    wy0, wy1 = (16 - fy).astype(np.float32)[:, None], fy.astype(np.float32)[:, None]
    wx0, wx1 = (16 - fx).astype(np.float32)[:, None], fx.astype(np.float32)[:, None]
    sixteen = np.float32(16)

    def row(y):
        a, b = images[f, y, ix], images[f, y, ix1]
        return np.where((fx == 0)[:, None], sixteen * a, (wx0 * a).astype(np.float32) + (wx1 * b).astype(np.float32)).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        top, bot = row(iy), row(iy1)
        v = np.where((fy == 0)[:, None], sixteen * top, (wy0 * top).astype(np.float32) + (wy1 * bot).astype(np.float32))
        return (v.astype(np.float32) * np.float32(1 / 256)).astype(np.float32)


def choose(t, known_t, org, source_t, nearer):
    """Where a pass writes frame t: masked pixels with an origin; the backward pass (`nearer`) only where nothing was found
    yet or its origin is strictly nearer in time."""
    write = (known_t == 0) & (org >= 0)
    if nearer:
        write &= (source_t == NONE) | (np.abs(t - org) < np.abs(t - source_t))
    return write


def temporal_fill_ref(images, mask, levels=4, search=2, smooth=8, reach=0, trace=None):
    """The whole call: (filled fp32 [F, H, W, C], remaining fp32 [F, H, W], source int32 [F, H, W]).  `trace`, a dict, receives
    per (direction, frame) the step's (vec, org, pos)."""
    images = np.asarray(images, dtype=np.float32)
    F, H, W = images.shape[:3]
    known = known_bits(np.asarray(mask, dtype=np.float32), F)
    Y = ref.luma(images)
    pyr = [ref.pyramid(Y[f], levels, ref.down_luma) for f in range(F)]
    kpyr = known_pyramids(known, levels)
    frames = np.arange(F)[:, None, None]
    source = np.where(known != 0, frames, NONE).astype(np.int64)
    filled = images.copy()
    for d in (1, -1):
        order = list(range(F)) if d == 1 else list(range(F - 1, -1, -1))
        state = None
        for donor, t in zip(order, order[1:]):
            vec = step_field(pyr[t], pyr[donor], kpyr[t], search, smooth)
            state = carry(t, known[t], donor, known[donor], vec, state, reach)
            org, pos = state
            write = choose(t, known[t], org, source[t], d == -1)
            filled[t][write] = sample(images, org[write], pos[write][:, 0], pos[write][:, 1])
            source[t][write] = org[write]
            if trace is not None:
                trace[(d, t)] = (vec, org, pos)
    remaining = ((known == 0) & (source == NONE)).astype(np.float32)
    return filled, remaining, source.astype(np.int32)
