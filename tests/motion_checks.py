"""Stage checks of the motion modules that a feature's own test and the scratch and long-clip tests both run."""
import numpy as np
import torch

from lanpaint_amd import (_cabi, propagate, propagate_anchored, propagate_anchored_visible, propagate_keys, shots, temporal_fill as tf,
                          temporal_fill_checked as tc)
from tests import propagate_ref as ref
from tests import propagate_visible_ref as vref
from tests import shots_ref as sref
from tests import temporal_fill_ref as tref
from tests.compare import _same_ints, _same_values
from tests.device import DEV, _dev, _equal
from tests.inputs import (ANCHORED_VISIBLE_LEVELS, FILL_FRAMES, FILL_LEVELS, KEYS_JOB_MASKS, KEYS_PARAMS, MASKS, VIDEOS, _carry_case,
                          _flags, _random_masks, _rng, _video)
from tests.temporal_clips import pair_case, pair_want


def _packed(planes, H, W, levels):
    """numpy planes of one frame's pyramid -> the device's byte string."""
    row = np.zeros(_cabi.prop_pyramid_ws_bytes(1, H, W, levels), np.uint8)
    for lv, p in enumerate(planes):
        off = _cabi.prop_level_offset(H, W, lv)
        row[off:off + p.size] = p.reshape(-1)
    return _dev(row)


def _check_match(H, W, levels, search, smooth, video, mask, what):
    images = VIDEOS[video](2, H, W, 3, seed=search)
    Y = ref.luma(images)
    ps, pt = (ref.pyramid(Y[f], levels, ref.down_luma) for f in range(2))
    pm = ref.pyramid(ref.binarise(MASKS[mask](H, W)), levels, ref.down_mask)
    src, tgt, mpyr = (_packed(p, H, W, levels) for p in (ps, pt, pm))
    _, trace = ref.motion_field(ps, pt, pm, search, smooth)
    for lv in range(levels - 1, -1, -1):
        raw, valid, final = trace[lv]
        parent = None if lv == levels - 1 else _dev(trace[lv + 1][2].astype(np.int32))
        vec, ok = propagate.match_level(src, tgt, mpyr, H, W, levels, lv, search, smooth, parent)
        _same_ints(ok.cpu().numpy(), valid, (what, "valid", lv))
        _same_ints(vec.cpu().numpy(), raw, (what, "vec", lv))
        _same_ints(propagate.fill_median(vec, ok).cpu().numpy(), final, (what, "fill and median", lv))
    return trace


def _anchored_field(P, Yt, Yk, m, anchor, smooth):
    vec, valid = propagate_anchored.anchor_field(_dev(P.astype(np.int32)), _dev(Yt), _dev(Yk), _dev(m), anchor, smooth)
    assert vec.dtype == valid.dtype == torch.int32 and tuple(valid.shape) == ref.grid_of(*Yt.shape) and tuple(vec.shape) == (*valid.shape, 2), (
        "vec and valid: int32, the block grid's shape")
    return vec.cpu().numpy(), valid.cpu().numpy()


def _anchored_visible_field(P, Yt, Yk, m, anchor, smooth, occlusion):
    vec, valid, gated = propagate_anchored_visible.gated_anchor_field(_dev(P.astype(np.int32)), _dev(Yt), _dev(Yk), _dev(m), anchor,
                                                                      smooth, occlusion)
    assert vec.dtype == valid.dtype == gated.dtype == torch.int32, "vec.dtype == valid.dtype == gated.dtype == torch.int32"
    assert tuple(valid.shape) == tuple(gated.shape) == ref.grid_of(*Yt.shape) and tuple(vec.shape) == (*valid.shape, 2), (
        "valid and gated on the block grid, vec with two components")
    return vec.cpu().numpy(), valid.cpu().numpy(), gated.cpu().numpy()


def _anchored_visible_call(images, mask, key, anchor=2, occlusion=16):
    return propagate_anchored_visible.propagate_masks_anchored_visible(images, mask, key, ANCHORED_VISIBLE_LEVELS, 2, 8, anchor, occlusion)


def _check_batched_entries(plane, jobs):
    H, W = plane
    images = _dev(_video(jobs + 1, H, W, 3, seed=jobs))
    rng = _rng(H, W, jobs)
    for levels, search, smooth in KEYS_PARAMS:
        pyr = propagate.luma_pyramids(images, levels)
        keys = [propagate.key_mask(_dev(MASKS[KEYS_JOB_MASKS[i % len(KEYS_JOB_MASKS)]](H, W, i)), levels)[0] for i in range(jobs)]
        pos = [None if i % 2 == 0 else _dev(np.maximum(ref.key_positions(H, W) + rng.integers(-40, 41, (H, W, 2)), 0).astype(np.int32))
               for i in range(jobs)]
        single, parents = [], [None] * jobs
        for i in range(jobs):
            trace, parent = [], None
            for lv in range(levels - 1, -1, -1):
                vec, valid = propagate.match_level(pyr[i], pyr[i + 1], keys[i], H, W, levels, lv, search, smooth, parent)
                parent = propagate.fill_median(vec, valid)
                trace.append((vec, valid, parent))
            bits = propagate.level_view(keys[i], H, W, 0)[0]
            single.append((trace, propagate.advance(parent, pos[i], bits, levels)))
        for n, lv in enumerate(range(levels - 1, -1, -1)):
            got = propagate_keys.match_level_batch([(pyr[i], pyr[i + 1], keys[i], parents[i]) for i in range(jobs)], H, W, levels, lv,
                                                   search, smooth)
            parents = propagate_keys.fill_median_batch(got)
            for i in range(jobs):
                what = (plane, jobs, levels, "level", lv, "job", i)
                _equal(got[i][0], single[i][0][n][0], (*what, "vec"))
                _equal(got[i][1], single[i][0][n][1], (*what, "valid"))
                _equal(parents[i], single[i][0][n][2], (*what, "field"))
        got = propagate_keys.advance_batch([(parents[i], pos[i], propagate.level_view(keys[i], H, W, 0)[0]) for i in range(jobs)], levels)
        for i in range(jobs):
            for g, w, name in zip(got[i][:2], single[i][1][:2], ("positions", "mask")):
                _equal(g, w, (plane, jobs, levels, "job", i, name))
            for lv in range(levels):                                  # the bytes between two levels belong to nobody
                _equal(propagate.level_view(got[i][2], H, W, lv), propagate.level_view(single[i][1][2], H, W, lv),
                       (plane, jobs, levels, "job", i, "pyramid level", lv))


def _offset_view(a, offset, stride=None):
    """`a` on the device as a view `offset` bytes into a buffer of its own, as one row of `stride` elements if given (the rest of
    a pyramid row: 0xA5, which nobody may read)."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    n = t.numel() if stride is None else stride
    buf = torch.full((offset // t.element_size() + n,), 0xA5 if t.dtype == torch.uint8 else -1, dtype=t.dtype, device=DEV)
    view = buf[offset // t.element_size():]
    view[:t.numel()] = t.reshape(-1).to(DEV)
    return view if stride is not None else view.view(a.shape)


def _merge_inputs(H, W, span, flag_kind):
    n = span - 1
    gh, gw = ref.grid_of(H, W)
    rng = _rng(H, W, span, 31)
    q = rng.integers(-12, 13, (2, n, H, W))
    far = rng.random((2, n, H, W))
    q = np.where(far < 0.2, rng.integers(-5000, 5001, (2, n, H, W)), q)
    q = np.where(far > 0.95, np.where(q < 0, -_cabi.LP_STAB_Q_FAR, _cabi.LP_STAB_Q_FAR), q)
    c = rng.integers(0, 257, (2, n, H, W))
    c[rng.random((2, n, H, W)) < 0.3] = 256
    if flag_kind == "random":
        f = rng.integers(0, 2, (2, n, gh, gw))
    else:                                                              # the forward chain's as named, the backward chain's the opposite
        f = np.stack([np.stack([_flags(flag_kind, gh, gw)] * n), np.stack([1 - _flags(flag_kind, gh, gw)] * n)])
    g = rng.integers(0, 2, (2, n, gh, gw))                             # any visible part c' <= c will do for the chains' own masks
    cv = np.stack([np.stack([vref.occlude(c[x, i], g[x, i]) for i in range(n)]) for x in range(2)])
    return q, c, cv, f


def _check_scores(images, level, search, what):
    score, n = shots.shot_scores(_dev(images), level, search)
    want, want_n = sref.shot_scores(images, level, search)
    assert n == want_n and score.is_cuda and score.dtype == torch.int64 and score.is_contiguous() and tuple(score.shape) == want.shape, (
        "the pair count and score: on the device, int64, contiguous, the restatement's shape")
    _same_ints(score.cpu().numpy(), want, what)
    return want


def _check_batched_fields():
    frames, H, W = 18, 23, 33
    images, mask = _video(frames, H, W), _random_masks(frames, H, W)
    luma = propagate.luma_pyramids(_dev(images), FILL_LEVELS)
    known = tf.known_pyramids(_dev(mask), frames, FILL_LEVELS)
    steps = [(t, t - 1) for t in range(1, frames)] + [(t, t + 1) for t in range(frames - 2, -1, -1)]
    assert len(steps) == 34 and len(steps) % tf.MAX_JOBS == 2, "34 steps, two over a launch"      # two launches per level, a remainder of 2
    got = tf.step_fields(luma, known, steps, H, W, FILL_LEVELS, 2, 8)
    assert got.dtype == torch.int32 and tuple(got.shape) == (34, *_cabi.prop_grid(H, W), 2), "the step fields: int32 [34, grid, 2]"
    Y = ref.luma(images)
    pyr = [ref.pyramid(Y[f], FILL_LEVELS, ref.down_luma) for f in range(frames)]
    kpyr = tref.known_pyramids(tref.known_bits(mask, frames), FILL_LEVELS)
    host = got.cpu().numpy()
    for j, (t, s) in enumerate(steps):
        parent = None
        for lv in range(FILL_LEVELS - 1, -1, -1):
            vec, ok = propagate.match_level(luma[t], luma[s], known[t], H, W, FILL_LEVELS, lv, 2, 8, parent)
            parent = propagate.fill_median(vec, ok)
        assert torch.equal(got[j], parent), ("the single entries", j, t, s)
        _same_ints(host[j], tref.step_field(pyr[t], pyr[s], kpyr[t], 2, 8), ("the restatement", j, t, s))


def _check_carry(H, W, wild, donor, state, reach, nearer, channels=3):
    t = 2
    images, vec, known, org, pos, source_t = _carry_case(H, W, wild, channels)
    known_t, known_s = known[1], known[donor - 1]
    want_org, want_pos = tref.carry(t, known_t, donor, known_s, vec, (org, pos) if state else None, reach)
    write = tref.choose(t, known_t, want_org, source_t, nearer)
    source = np.full((FILL_FRAMES, H, W), -7, np.int32)
    source[t] = source_t
    remaining = np.full((FILL_FRAMES, H, W), 0.25, np.float32)
    remaining[t] = (known_t == 0) & (source_t == -1)
    filled = images.copy()
    want_filled, want_source, want_remaining = filled.copy(), source.copy(), remaining.copy()
    want_filled[t][write] = tref.sample(images, want_org[write], want_pos[write][:, 0], want_pos[write][:, 1])
    want_source[t][write] = want_org[write]
    want_remaining[t][write] = 0
    d_filled, d_source, d_remaining = _dev(filled), _dev(source), _dev(remaining)
    got_org, got_pos = tf.carry(_dev(vec), _dev(known_t), _dev(known_s), (_dev(org), _dev(pos)) if state else None, _dev(images),
                                d_filled, d_source, d_remaining, t, donor, reach, nearer)
    what = ((H, W), wild, donor, state, reach, nearer, channels)
    under = known_t == 0                                               # the state planes matter under the mask only
    _same_ints(got_org.cpu().numpy()[under], want_org[under], (what, "org"))
    _same_ints(got_pos.cpu().numpy()[under], want_pos[under], (what, "pos"))
    _same_values(d_filled.cpu().numpy(), want_filled, (what, "filled"))
    _same_ints(d_source.cpu().numpy(), want_source, (what, "source"))
    _same_values(d_remaining.cpu().numpy(), want_remaining, (what, "remaining"))
    return want_org, write


def _check_fill_whole(got, want, what):
    for g, dtype in zip(got, (torch.float32, torch.float32, torch.int32)):
        assert g.is_cuda and g.dtype == dtype and g.is_contiguous(), "g.is_cuda and g.dtype == dtype and g.is_contiguous()"
    _same_values(got[0].cpu().numpy(), want[0], (what, "filled"))
    _same_values(got[1].cpu().numpy(), want[1], (what, "remaining"))
    _same_ints(got[2].cpu().numpy(), want[2], (what, "source"))


def _check_pair(H, W, wild, C, state, reach, agree):
    t = 2
    case = pair_case(H, W, wild, C)
    images, vec, known, org, pos, source_t, filled_t = case
    (want_org, want_pos), want = pair_want(case, state, reach, agree)
    filled, source = images.copy(), np.full((FILL_FRAMES, H, W), -7, np.int32)
    remaining, witnesses = np.full((FILL_FRAMES, H, W), 0.25, np.float32), np.full((FILL_FRAMES, H, W), 77, np.int32)
    filled[t], source[t], remaining[t] = filled_t, source_t, (known[0] == 0) & (source_t == -1)
    wants = [filled.copy(), source.copy(), remaining.copy(), witnesses.copy()]
    for plane, w in zip(wants, want):
        plane[t] = w
    d_filled, d_source, d_remaining, d_witnesses = _dev(filled), _dev(source), _dev(remaining), _dev(witnesses)
    got_org, got_pos = tc.carry_pair(_dev(vec), _dev(known[0]), _dev(known[1]), (_dev(org), _dev(pos)) if state else None,
                                     _dev(images), d_filled, d_source, d_remaining, d_witnesses, t, reach, agree)
    what = ((H, W), wild, C, state, reach, agree)
    under = known[0] == 0                                              # the state planes matter under the mask only
    _same_ints(got_org.cpu().numpy()[under], want_org[under], (what, "org"))
    _same_ints(got_pos.cpu().numpy()[under], want_pos[under], (what, "pos"))
    _same_values(d_filled.cpu().numpy(), wants[0], (what, "filled"))
    _same_ints(d_source.cpu().numpy(), wants[1], (what, "source"))
    _same_values(d_remaining.cpu().numpy(), wants[2], (what, "remaining"))
    _same_ints(d_witnesses.cpu().numpy(), wants[3], (what, "witnesses"))


def _check_checked_whole(got, want, what):
    for g, dtype in zip(got, (torch.float32, torch.float32, torch.int32, torch.int32)):
        assert g.is_cuda and g.dtype == dtype and g.is_contiguous(), "g.is_cuda and g.dtype == dtype and g.is_contiguous()"
    _same_values(got[0].cpu().numpy(), want[0], (what, "filled"))
    _same_values(got[1].cpu().numpy(), want[1], (what, "remaining"))
    _same_ints(got[2].cpu().numpy(), want[2], (what, "source"))
    _same_ints(got[3].cpu().numpy(), want[3], (what, "witnesses"))


def _check_smooth(got, want, what):
    out, support = got
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and support.dtype == torch.int32 and support.is_contiguous(), (
        "out: device fp32 contiguous; support: int32 contiguous")
    _same_ints(support.cpu().numpy(), want[1], (what, "support"))
    _same_values(out.cpu().numpy(), want[0], (what, "out"))


def _check_robust_smooth(got, want, what):
    out, support, replaced = got
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous(), "out: on the device, fp32, contiguous"
    for plane in (support, replaced):
        assert plane.dtype == torch.int32 and plane.is_contiguous() and plane.shape == out.shape[:3], (
            "support and replaced: int32, contiguous, one value per pixel")
    _same_ints(support.cpu().numpy(), want[1], (what, "support"))
    _same_ints(replaced.cpu().numpy(), want[2], (what, "replaced"))
    _same_values(out.cpu().numpy(), want[0], (what, "out"))
