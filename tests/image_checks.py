"""Stage checks of the image-space modules that a feature's own test and the scratch tests both run."""
import numpy as np
import torch

from lanpaint_amd import _cabi, detail, detail_color, grain, stabilize, videomask
from lanpaint_amd.videomask import FRAME_DTYPE
from tests import color_ref, grain_ref, stabilize_ref
from tests import videomask_ref as vref
from tests.compare import _same_raw_bits, _same_typed
from tests.device import DEV, _dev, _gen
from tests.image_inputs import _m3, _row


def _bbox_ref(mask):
    m = mask if mask.ndim == 3 else mask.unsqueeze(0)
    nz = torch.nonzero(m > 0.5)
    if nz.shape[0] == 0:
        return (m.shape[1], -1, m.shape[2], -1)
    return (int(nz[:, 1].min()), int(nz[:, 1].max()), int(nz[:, 2].min()), int(nz[:, 2].max()))


def _region(y0, x0, hw, out_hw, H, W):
    return detail.Region(y0, x0, hw[0], hw[1], out_hw[0], out_hw[1], H, W)


def _rect_mask(shape, rects, soft_seed=None):
    mask = torch.zeros(shape)
    for f, y0, y1, x0, x1 in rects:
        mask[f, y0:y1 + 1, x0:x1 + 1] = 1.0
    if soft_seed is not None:                                              # soft values above 0.5 inside, below outside
        noise = torch.rand(shape, generator=_gen(soft_seed))
        mask = torch.where(mask > 0, 0.55 + 0.45 * noise, 0.3 * noise * (noise > 0.8))
    return mask


def _outside_is_untouched(out, original, r):
    probe = out.clone()
    probe[:, r.y0:r.y0 + r.h, r.x0:r.x0 + r.w, :] = original[:, r.y0:r.y0 + r.h, r.x0:r.x0 + r.w, :]
    return torch.equal(probe, original)


def _check_color_stats(d, r, mask, margin, what):
    """Device stats of CPU arrays against the restatement; returns the device table."""
    dt, rt = torch.from_numpy(d).to(DEV), torch.from_numpy(r).to(DEV)
    mt = None if mask is None else torch.from_numpy(mask).to(DEV)
    got_dev = detail_color.color_stats(dt, rt, mt, margin)
    again = detail_color.color_stats(dt, rt, mt, margin)
    assert got_dev.dtype == torch.float64 and tuple(got_dev.shape) == (d.shape[0], 1 + 4 * d.shape[3]), (
        "the statistics' dtype (float64) and shape [B, 1 + 4 C]")
    got = got_dev.cpu().numpy()
    assert (got.view(np.uint64) == again.cpu().numpy().view(np.uint64)).all(), what          # two calls, equal bits
    want, mag = color_ref.stats_ref(d, r, mask, margin)
    assert (got[:, 0] == want[:, 0]).all(), (what, got[:, 0], want[:, 0])                   # n exactly
    bound = want[:, :1] * 2.0 ** -52 * mag[:, 1:]
    err = np.abs(got[:, 1:] - want[:, 1:])
    assert (err <= bound).all(), (what, float((err / np.maximum(bound, 1e-300)).max()))
    return got_dev


def _fit_bits(stats, *args):
    got = detail_color.color_fit(stats, *args).cpu().numpy()
    want = color_ref.fit_ref(stats.cpu().numpy(), *args)
    assert got.dtype == np.float32 and got.shape == want.shape, "got.dtype == np.float32 and got.shape == want.shape"
    assert (got.view(np.uint32) == want.view(np.uint32)).all(), (args, got[got != want][:4], want[got != want][:4])
    return got


def _window_mask(track):
    inside = torch.zeros(len(track), track.H, track.W, dtype=torch.bool)       # built on the CPU, frame by frame
    for f, (y0, x0) in enumerate(track.origins):
        inside[f, y0:y0 + track.h, x0:x0 + track.w] = True
    return inside


def _check_grain_stats(image, mask, cases, what):
    t_img, t_mask = _dev(image), _dev(mask)
    got = torch.stack([grain.grain_stats(t_img, t_mask, r, f, m) for r, f, m in cases]).cpu().numpy()
    for g, (r, f, m) in zip(got, cases):
        _same_typed(g, grain_ref.grain_stats(image, _m3(mask), grain.REGIONS[r], f, m), (what, r, f, m))
    return got


def _check_fit(gen, reft, cases, what):
    for strength, size, clip in cases:
        amp, sz = grain.grain_fit(_dev(gen), _dev(reft), strength, size, clip)
        assert amp.is_cuda and sz.is_cuda and sz.dtype == torch.int32, "amp.is_cuda and sz.is_cuda and sz.dtype == torch.int32"
        want_amp, want_size = grain_ref.grain_fit(gen, reft, strength, size, clip)
        _same_typed(sz.cpu().numpy(), want_size, (what, "size", strength, size, clip))
        _same_typed(amp.cpu().numpy(), want_amp, (what, "amp", strength, size, clip))
    return want_amp, want_size


def _device_q(mask):
    return stabilize.signed_d2(torch.from_numpy(mask).to(DEV))


def _check_q(q_dev, q_ref, cases, what):
    """Every (median, smooth, grow, feather) of `cases` on the device's q against the restatement on its own q; the device's
    results come back in one copy."""
    got = torch.stack([stabilize.stabilize_q(q_dev, *c) for c in cases]).cpu().numpy()
    for g, c in zip(got, cases):
        _same_raw_bits(g, stabilize_ref.stabilize_q_ref(q_ref, *c), (what, c))
    return got


EDT_NONE = _cabi.LP_VMASK_D2_NONE


def _brute_d2(fg):
    """Squared distance to the nearest True pixel by brute force, -1 where there is none."""
    h, w = fg.shape
    ys, xs = np.nonzero(fg)
    if len(ys) == 0:
        return np.full((h, w), EDT_NONE, np.int64)
    yy, xx = np.mgrid[:h, :w]
    out = np.full((h, w), np.iinfo(np.int64).max, np.int64)
    for c in range(0, len(ys), 256):
        d = (yy[..., None] - ys[c:c + 256]) ** 2 + (xx[..., None] - xs[c:c + 256]) ** 2
        out = np.minimum(out, d.min(-1))
    return out


def _edt(masks):
    keys = torch.from_numpy(np.ascontiguousarray(np.stack(masks)).astype(np.float32)).to(DEV)
    d2, sdf, csum = videomask.keyframe_edt(keys)
    torch.cuda.synchronize()
    return d2.cpu().numpy(), sdf.cpu().numpy(), csum.cpu().numpy()


def _check_edt(masks):
    d2, sdf, csum = _edt(masks)
    for k, m in enumerate(masks):
        fg = np.asarray(m) >= 0.5
        assert np.array_equal(d2[k, 0], _brute_d2(fg)), k
        assert np.array_equal(d2[k, 1], _brute_d2(~fg)), k
        ys, xs = np.nonzero(fg)
        assert csum[k].tolist() == [len(ys), int(ys.sum()), int(xs.sum())], "csum[k].tolist() == [len(ys), int(ys.sum()), int(xs.sum())]"
        h, w = fg.shape
        if not fg.any() or fg.all():
            assert (sdf[k] == (max(h, w) / 2.0) * (1 if fg.all() else -1)).all(), (
                "the signed distance of a constant plane against +-max(h, w) / 2")
        else:
            assert np.array_equal(sdf[k], np.sqrt(d2[k, 1].astype(np.float64)) - np.sqrt(d2[k, 0].astype(np.float64))), (
                "the signed distance against sqrt(d2 to background) - sqrt(d2 to foreground)")


PLAN_ZERO, PLAN_KEY, PLAN_INNER = _cabi.LP_VMASK_ZERO, _cabi.LP_VMASK_KEY, _cabi.LP_VMASK_INNER


def _hand_plan(h, w, n_keys):
    """(plan, indices of the fully vacated INNER frames, indices of the entries naming a key out of range)."""
    third, big = 1.0 / 3.0, 2 ** 31 - 1
    rows = [
        _row(PLAN_INNER, 0, 1, wf=third),                                                          # 0: no shift
        _row(PLAN_INNER, 0, 1, sy1=1, sx1=-1, sy2=1, sx2=-1, wf=third),                            # 1, 2: one pixel
        _row(PLAN_INNER, 0, 1, sy1=-1, sx1=1, sy2=-1, sx2=1, wf=0.5),
        _row(PLAN_ZERO),
        _row(PLAN_INNER, 0, 1, sy1=h - 1, sx1=w - 1, sy2=h - 1, sx2=w - 1, wf=third),              # 4, 5: one row / column is left
        _row(PLAN_INNER, 0, 1, sy1=1 - h, sx1=1 - w, sy2=1 - h, sx2=1 - w, wf=third),
        _row(PLAN_INNER, 0, 1, sy1=h, sy2=h, wf=third),                                            # 6: past the frame in y only
        _row(PLAN_INNER, 0, 1, sx1=-w, sx2=-w, wf=third),                                          # 7: in x only
        _row(PLAN_INNER, 0, 1, sy1=h + 3, sx1=w, sy2=-h, sx2=-(w + 7), wf=third),                  # 8: in both
        _row(PLAN_INNER, 1, 0, sy1=big, sx1=-big - 1, sy2=-big - 1, sx2=big, wf=0.25),             # 9: the largest integers
        _row(PLAN_INNER, 0, 1, sy1=2, sx1=-2, sy2=-3, sx2=1, wf=third),                            # 10: both keys move the same way
        _row(PLAN_INNER, 0, 1, sy1=-1, sx1=5, sy2=4, sx2=-2, wf=0.75),                             # 11: mixed signs per axis
        _row(PLAN_INNER, 0, 1, wf=0.0), _row(PLAN_INNER, 0, 1, wf=1.0),                                 # 12, 13: the end weights
        _row(PLAN_INNER, 0, 1, sy1=h, wf=third),                                                   # 14: only one key vacated
        _row(PLAN_KEY, 2),
        _row(PLAN_INNER, 0, 3, sx1=1, wf=third), _row(PLAN_INNER, 2, 2, sy1=1, wf=third),               # 16, 17: not adjacent; equal
        _row(PLAN_INNER, 4, 1, sx2=1, wf=third), _row(PLAN_INNER, 3, 4, wf=0.5),                        # 18, 19: hi < lo; empty to full
        _row(PLAN_ZERO),
        _row(PLAN_INNER, -1, 1, wf=third), _row(PLAN_INNER, 0, n_keys, wf=third),                       # 21 .. 25: no such key
        _row(PLAN_KEY, -1), _row(PLAN_KEY, n_keys), _row(PLAN_INNER, n_keys, -1, wf=third),
        _row(PLAN_KEY, 0), _row(PLAN_KEY, n_keys - 1), _row(PLAN_ZERO),
    ]
    return np.array(rows, FRAME_DTYPE), [6, 7, 8, 9], [21, 22, 23, 24, 25]


def _check_morph(tag, keys, stack, sdf, plan):
    """The device's float and codes output of `plan` against the arbiter; returns (got, codes, want)."""
    want = vref.morph_ref(keys, plan)
    got = videomask.morph_frames(stack, plan, sdf).cpu().numpy()
    codes = videomask.morph_frames(stack, plan, sdf, codes=True).cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32 and codes.dtype == np.uint8, (
        "the morph's shape and fp32 dtype, the codes' uint8 dtype")
    ulp = vref.ulp_diff(got, want)
    differing = int(np.count_nonzero(got.view(np.uint32) != want.view(np.uint32)))
    h, w = keys.shape[1:]
    print(f"VMASK_MORPH {h}x{w} {tag}: max ulp {int(ulp.max())}, differing {differing} of {got.size}")
    assert ulp.max() <= 1, int(ulp.max())
    assert 1.0 - differing / got.size >= 0.99999, (differing, got.size)
    assert np.array_equal(codes, vref.codes_ref(got)), "the codes against the codes of the morph"  # the conversion alone: the same fp32 multiply
    want_codes = vref.codes_ref(want)
    assert np.abs(codes.astype(np.int16) - want_codes.astype(np.int16)).max() <= 1, (
        "the device's codes within one code of the float64 plan's")
    for t, p in enumerate(plan):                                         # what holds exactly
        if p["kind"] == PLAN_ZERO:
            assert not got[t].any() and not codes[t].any(), t
        elif p["kind"] == PLAN_KEY and 0 <= p["key_lo"] < len(keys):
            assert np.array_equal(got[t].view(np.uint32), keys[p["key_lo"]].view(np.uint32)), t
    return got, codes, want
