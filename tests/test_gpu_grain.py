"""The grain match on the MI355X (lanpaint_amd.grain, csrc/grain_kernel.hip) against the numpy restatement tests/grain_ref.py.
The rule is integers, then fp64 and fp32 with every operation rounded on its own, so the device must give the restatement's bits
whatever tile, block or chunk a launch uses: every comparison covers every element and has no tolerance."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, grain, grain_nodes
from lanpaint_amd._util import raw_stream
from tests import grain_ref as ref
from tests.compare import _raw_bits as _bits, _same_typed as _same
from tests.device import DEV, _dev
from tests.image_checks import _check_fit, _check_grain_stats as _check_stats
from tests.image_inputs import IMAGES, _box, _grain_wild as _wild, _m3, _named_rng as _rng, _random_table

pytestmark = pytest.mark.gpu
TH, TW = _cabi.LP_GRAIN_TILE_H, _cabi.LP_GRAIN_TILE_W                  # 16 x 64
# (B, H, W, C): one pixel; no interior pixel; exactly one; odd sizes; one under, at and one over the tile's width and height
# and the four channels of a group; 16 Philox blocks per pixel; several tiles each way
SHAPES = [(1, 1, 1, 1), (1, 4, 9, 1), (1, 5, 5, 1), (2, 7, 9, 3), (3, 6, TW - 1, 4), (3, 6, TW, 5), (3, 6, TW + 1, 4),
          (1, TH - 1, TW - 1, 2), (1, TH, TW, 3), (1, TH + 1, TW + 1, 3), (2, 40, 70, 64), (5, 70, 130, 3)]
IDS = lambda s: "x".join(map(str, s))                                  # noqa: E731
BIG_SEED = (1 << 63) + 5


# ---- masks ----------------------------------------------------------------------------------------------------------------------------
def _soft(B, H, W, seed=4):
    rng = _rng(B, H, W, seed)
    yy, xx = np.mgrid[:H, :W]
    m = np.clip(1.3 - np.hypot(yy - H / 2, xx - W / 2) / (0.3 * max(H, W) + 1), 0, 1)[None] * np.ones((B, 1, 1))
    return (m + 0.01 * rng.random((B, H, W))).astype(np.float32)       # a little over 1 at the centre: clamped


def _wild_mask(B, H, W, seed=5):
    return _wild(B, H, W, 1, seed)[..., 0]


MASKS = {"[H, W]": lambda B, H, W: _box(B, H, W, False)[0], "[1, H, W]": lambda B, H, W: _box(B, H, W, False), "[B, H, W]": _box,
         "soft": _soft, "empty": lambda B, H, W: np.zeros((B, H, W), np.float32), "full": lambda B, H, W: np.ones((B, H, W), np.float32),
         "wild": _wild_mask}


# ---- stats ----------------------------------------------------------------------------------------------------------------------------
STATS_CASES = [("all", 0, 8), ("all", 1, 8), ("all", 64, 8), ("all", 255, 8), ("outside", 64, 0), ("outside", 255, 1),
               ("outside", 64, 25), ("outside", 255, 8), ("inside", 64, 8), ("inside", 255, 8), ("inside", 1, 8)]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_stats_equal_the_restatement(shape):
    B, H, W, C = shape
    for form, mform in (("medium", "[B, H, W]"), ("boundaries", "soft")):
        got = _check_stats(IMAGES[form](B, H, W, C), MASKS[mform](B, H, W), STATS_CASES, (shape, form))
        if H < 5 or W < 5:
            assert not got.any()
        elif form == "medium":
            assert got[3, ..., 0].sum() == B * C * (H - 4) * (W - 4)   # "all" at flat 255 takes every interior pixel


@pytest.mark.parametrize("form", list(IMAGES))
def test_every_image_form_through_stats_and_apply(form):
    B, H, W, C = 2, 33, 70, 3
    image, mask = IMAGES[form](B, H, W, C), _soft(B, H, W)
    got = _check_stats(image, mask, STATS_CASES, form)
    if form == "checker":
        assert not got[:3].any() and got[3].any()                       # flat rejects everything below 255
    if form in ("all 0", "all 1"):
        assert not got[..., 1:].any() and got[3, ..., 0 if form == "all 0" else 7, 0].all()
    rng = _rng(form, 7)
    amp = (rng.random((B, C, ref.K)) * 2e-4).astype(np.float32)
    sizes = np.array([2, 1], np.int32)
    out = grain.grain_apply(_dev(image), _dev(mask), _dev(amp), _dev(sizes), seed=3, frame0=2).cpu().numpy()
    _same(out, ref.grain_apply(image, mask, amp, sizes, 3, False, 2), (form, "apply"))


@pytest.mark.parametrize("mform", list(MASKS))
def test_every_mask_form_through_stats_apply_and_match(mform):
    B, H, W, C = 3, 37, 75, 3
    image, mask = IMAGES["coarse"](B, H, W, C), MASKS[mform](B, H, W)
    _check_stats(image, mask, STATS_CASES[4:], mform)
    amp = (_rng(mform, 8).random((B, C, ref.K)) * 2e-4).astype(np.float32)
    amp[0, 0, 3] = 0.0
    sizes = np.array([0, 2, 1], np.int32)
    out = grain.grain_apply(_dev(image), _dev(mask), _dev(amp), _dev(sizes), seed=BIG_SEED, monochrome=True).cpu().numpy()
    _same(out, ref.grain_apply(image, _m3(mask), amp, sizes, BIG_SEED, True), (mform, "apply"))
    keep = np.broadcast_to(ref.mask01(_m3(mask)) == 0, (B, H, W))
    assert (_bits(out)[keep] == _bits(image)[keep]).all()
    if mform == "empty":
        assert (_bits(out) == _bits(image)).all()
    if mform == "full":
        assert (out != image).mean() > 0.9
    got = grain.match(_dev(image), _dev(mask), flat=255, seed=1).cpu().numpy()
    _same(got, ref.match(image, _m3(mask), flat=255, seed=1), (mform, "match"))
    assert (_bits(got)[keep] == _bits(image)[keep]).all()


# ---- field ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_field_equals_the_restatement(shape):
    B, H, W, C = shape
    small = B * H * W * C <= 5000
    combos = [(m, f, s) for m in (False, True) for f in (0, 1000) for s in (0, BIG_SEED)] if small else \
        [(False, 0, 0), (True, 1000, BIG_SEED), (False, 1000, BIG_SEED)]
    for size in (0, 1, 2):
        got = torch.stack([grain.grain_field(shape, size, s, m, f, DEV) for m, f, s in combos]).cpu().numpy()
        for g, (m, f, s) in zip(got, combos):
            _same(g, ref.grain_field(B, H, W, C, size, s, m, f), (shape, size, m, f, s))


def test_field_in_two_chunks_is_the_field_of_the_whole_batch():
    shape = (5, 21, 70, 6)
    for size in (0, 1, 2):
        whole = grain.grain_field(shape, size, 9, False, 7, DEV)
        a, b = grain.grain_field((2,) + shape[1:], size, 9, False, 7, DEV), grain.grain_field((3,) + shape[1:], size, 9, False, 9, DEV)
        assert torch.equal(whole, torch.cat([a, b]))
        assert not torch.equal(whole[0], whole[1]) and not torch.equal(whole[..., 0], whole[..., 4])


def test_the_white_field_has_the_variance_the_fit_assumes():
    g = grain.grain_field((1, 256, 256, 3), 0, 21, False, 0, DEV).double()
    assert abs(float((g ** 2).mean()) - ref.WHITE_VAR) <= 0.02 * ref.WHITE_VAR and abs(float(g.mean())) < 3.0


# ---- fit ------------------------------------------------------------------------------------------------------------------------------
def _table(B, C, rows):
    t = np.zeros((B, C, ref.K, 3), np.int64)
    for (b, c, k), v in rows.items():
        t[b, c, k] = v
    return t


def test_fit_branches_equal_the_restatement():
    none = _table(1, 1, {(0, 0, 0): (63, 10 ** 6, 10 ** 6)})
    one = _table(1, 1, {(0, 0, 3): (64, 64 * 360, 64 * 360)})
    every = [(1.0, -1, 0), (0.0, -1, 0), (2.0, -1, 0), (0.37, 0, 0), (1.0, 1, 0), (1.5, 2, 0)]
    amp, _ = _check_fit(none, none, every, "no valid reference band")
    assert not amp.any()
    _check_fit(none, one, every, "no valid generated band, one valid reference band")
    amp, size = _check_fit(one, one, every[:1], "A <= 0")
    assert not amp.any() and size.tolist() == [0]
    amp, _ = _check_fit(one, one, [(1.0, 2, 0)], "nothing missing at a given size")
    assert not amp.any()
    ties = _table(1, 2, {(0, 0, 2): (64, 6400, 6400), (0, 0, 4): (70, 70000, 70000), (0, 1, 0): (64, 64, 64), (0, 1, 7): (64, 640, 640)})
    amp, _ = _check_fit(none.repeat(2, axis=1), ties, every, "ties")
    assert amp[0, 0, 3] == amp[0, 0, 2] != amp[0, 0, 4] and amp[0, 1, 3] == amp[0, 1, 0] and amp[0, 1, 4] == amp[0, 1, 7]
    for e1, e2, under, over in ((3000, 14000, 0, 1), (1000, 33000, 1, 2)):     # each size threshold: just under, at, just over
        for delta, want in ((-1, under), (0, over), (1, over)):
            t = _table(1, 1, {(0, 0, 5): (64, 64 * e1, 64 * e2 + delta)})
            _, size = _check_fit(none, t, [(1.0, -1, 0)], ("threshold", e1, e2, delta))
            assert size.tolist() == [want], (e1, e2, delta)
    loud = _table(1, 1, {(0, 0, 1): (100, 100 * 10 ** 9, 100 * 10 ** 9)})  # the MAX_STD cap, at every size
    for size in (0, 1, 2):
        amp, _ = _check_fit(none, loud, [(1.0, size, 0), (2.0, size, 0)], "cap")
        assert (amp == np.float32(64 / np.sqrt(ref.WHITE_VAR * ref.SUM_K2[size]) / 255.0)).all()


@pytest.mark.parametrize("C", [1, 3, 64])
def test_fit_pools_clips_and_plates_as_the_restatement_does(C):
    B = 12
    gen, same = _random_table(B, C, 1, 100), _random_table(B, C, 2)
    plate = _random_table(5, C, 3)
    cases = [(1.0, -1, 0), (1.0, -1, 1), (1.0, -1, 4), (0.8, -1, 12), (1.3, 1, 3), (1.0, 2, 6)]
    _, size = _check_fit(gen, same, cases[:3], ("Br == B", C))
    _check_fit(gen, same, cases[3:], ("Br == B", C))
    _check_fit(gen, plate, cases, ("Br != B", C))
    _check_fit(gen[:1], plate, cases[:2], ("one image", C))
    assert len(set(size.reshape(3, 4).tolist()[0])) == 1               # a clip shares its size


# ---- apply and match ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_apply_and_match_equal_the_restatement(shape):
    B, H, W, C = shape
    form = ("white", "medium", "coarse")[(H + W) % 3]
    image, mask = IMAGES[form](B, H, W, C), _box(B, H, W)
    image = image * (1.0 - 0.999 * mask[..., None]) + 0.999 * mask[..., None] * np.float32(0.5)      # clean under the mask
    image = image.astype(np.float32)
    rng = _rng(B, H, W, C, 11)
    amp = (rng.random((B, C, ref.K)) * 3e-4).astype(np.float32)
    sizes = rng.integers(0, 3, B).astype(np.int32)
    t_img, t_mask = _dev(image), _dev(mask)
    out = grain.grain_apply(t_img, t_mask, _dev(amp), _dev(sizes), seed=4, frame0=1000)
    _same(out.cpu().numpy(), ref.grain_apply(image, mask, amp, sizes, 4, False, 1000), (shape, "apply"))
    zero = grain.grain_apply(t_img, t_mask, _dev(np.zeros_like(amp)), _dev(sizes), seed=4)
    assert (_bits(zero.cpu().numpy()) == _bits(image)).all()
    got = grain.match(t_img, t_mask, flat=255, margin=2, seed=6)
    host = got.cpu().numpy()
    _same(host, ref.match(image, mask, flat=255, margin=2, seed=6), (shape, "match"))
    keep = mask == 0
    assert (_bits(host)[keep] == _bits(image)[keep]).all()
    assert torch.equal(grain.match(t_img, t_mask, flat=255, margin=2, seed=6), got)                 # two runs
    assert (_bits(grain.match(t_img, t_mask, strength=0.0, flat=255, margin=2).cpu().numpy()) == _bits(image)).all()


@functools.lru_cache(maxsize=None)
def _video():
    B, H, W, C = 6, 40, 90, 3
    image, mask = IMAGES["medium"](B, H, W, C), _box(B, H, W)
    clean = np.linspace(0.2, 0.8, W, dtype=np.float32)[None, None, :, None]
    image = np.where(mask[..., None] > 0.5, clean, image).astype(np.float32)
    return image, mask, IMAGES["coarse"](2, 50, 60, C, 9)


@pytest.mark.parametrize("kwargs", [dict(), dict(size="coarse", strength=1.7), dict(size=0, monochrome=True), dict(clip_frames=2),
                                    dict(clip_frames=1, flat=20, margin=0), dict(frame0=1000, seed=BIG_SEED, clip_frames=3)],
                         ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()) or "defaults")
def test_match_options_equal_the_restatement(kwargs):
    image, mask, plate = _video()
    want_kwargs = {**kwargs, "size": grain.SIZES.get(kwargs.get("size", "auto"), kwargs.get("size"))}
    got = grain.match(_dev(image), _dev(mask), **kwargs).cpu().numpy()
    _same(got, ref.match(image, mask, **want_kwargs), kwargs)
    assert (got != image).any()
    with_plate = grain.match(_dev(image), _dev(mask), _dev(plate), **kwargs).cpu().numpy()
    _same(with_plate, ref.match(image, mask, plate, **want_kwargs), ("plate", kwargs))


def test_chunks_give_the_bits_of_one_call(monkeypatch):
    image, mask, plate = _video()
    t_img, t_mask = _dev(image), _dev(mask)
    whole = grain.match(t_img, t_mask, seed=3, frame0=5, clip_frames=3)
    stats = grain.grain_stats(t_img, t_mask, "outside")
    per_frame = image[0].size * 4
    for frames in (1, 2, 4):
        monkeypatch.setattr(grain, "WS_CAP_BYTES", frames * per_frame + 8)
        assert [n for _, n in grain._frames(t_img)] == [frames] * (6 // frames) + ([6 % frames] if 6 % frames else [])
        assert torch.equal(grain.match(t_img, t_mask, seed=3, frame0=5, clip_frames=3), whole), frames
        assert torch.equal(grain.grain_stats(t_img, t_mask, "outside"), stats), frames
    monkeypatch.setattr(grain, "WS_CAP_BYTES", 1)                       # always at least one frame per chunk
    assert torch.equal(grain.match(t_img, t_mask, seed=3, frame0=5, clip_frames=3), whole)


def test_entries_stay_inside_their_outputs(hip_lib):
    B, H, W, C = 2, 19, 67, 5
    image, mask = IMAGES["medium"](B, H, W, C), _box(B, H, W)
    t_img, t_mask = _dev(image), _dev(mask)
    n, guard = B * H * W * C, 3
    amp = _dev((_rng(1).random((B, C, ref.K)) * 2e-4).astype(np.float32))
    sizes = _dev(np.array([2, 1], np.int32))
    buf = torch.full((n + 2 * guard,), float("nan"), dtype=torch.float32, device=DEV)
    d = _cabi.LpGrainApplyDesc(B, H, W, C, B, 0, 0, 7, t_img.data_ptr(), t_mask.data_ptr(), amp.data_ptr(), sizes.data_ptr(),
                               buf[guard:].data_ptr())
    assert hip_lib.lp_grain_apply(ctypes.byref(d), raw_stream(DEV)) == _cabi.LP_OK
    host = buf.cpu().numpy()
    assert np.isnan(host[:guard]).all() and np.isnan(host[guard + n:]).all(), "guard elements overwritten"
    _same(host[guard:guard + n].reshape(B, H, W, C), ref.grain_apply(image, mask, amp.cpu().numpy(), [2, 1], 7), "apply")
    ibuf = torch.full((n + 2 * guard,), 77, dtype=torch.int32, device=DEV)
    d = _cabi.LpGrainFieldDesc(B, H, W, C, 2, 0, 0, 7, ibuf[guard:].data_ptr())
    assert hip_lib.lp_grain_field(ctypes.byref(d), raw_stream(DEV)) == _cabi.LP_OK
    host = ibuf.cpu().numpy()
    assert (host[:guard] == 77).all() and (host[guard + n:] == 77).all(), "guard elements overwritten"
    _same(host[guard:guard + n].reshape(B, H, W, C), ref.grain_field(B, H, W, C, 2, 7), "field")
    rows = B * C * ref.K * 3
    sbuf = torch.full((rows + 2 * guard,), 77, dtype=torch.int64, device=DEV)
    d = _cabi.LpGrainStatsDesc(B, H, W, C, B, 1, 255, _cabi.LP_GRAIN_REGION_INSIDE, t_img.data_ptr(), t_mask.data_ptr(),
                               sbuf[guard:].data_ptr())
    assert hip_lib.lp_grain_stats(ctypes.byref(d), raw_stream(DEV)) == _cabi.LP_OK
    host = sbuf.cpu().numpy()
    assert (host[:guard] == 77).all() and (host[guard + rows:] == 77).all(), "guard elements overwritten"
    _same(host[guard:guard + rows].reshape(B, C, ref.K, 3), ref.grain_stats(image, mask, ref.INSIDE, 255), "stats")


def test_wrapper_takes_views_and_half_precision():
    image, mask, _ = _video()
    t_img, t_mask = _dev(image), _dev(mask)
    view = t_img[:, :, ::2]
    got = grain.match(view, t_mask[:, :, ::2], seed=2)
    _same(got.cpu().numpy(), ref.match(np.ascontiguousarray(image[:, :, ::2]), np.ascontiguousarray(mask[:, :, ::2]), seed=2), "a view")
    half = t_img.to(torch.float16)
    got = grain.match(half, t_mask, seed=2)
    assert got.dtype == torch.float32 and got.is_cuda
    _same(got.cpu().numpy(), ref.match(half.float().cpu().numpy(), mask, seed=2), "fp16")
    for bad in (t_img[0], t_img[:0], t_img[:, :, :, :0]):
        with pytest.raises(ValueError):
            grain.match(bad, t_mask)
    with pytest.raises(ValueError):
        grain.match(t_img, t_mask[:4])
    with pytest.raises(ValueError):
        grain.match(t_img, t_mask, t_img[..., :2])                       # another channel count
    with pytest.raises(ValueError):
        grain.match(t_img, t_mask, clip_frames=4)                        # does not divide 6
    with pytest.raises(ValueError):
        grain.grain_stats(t_img, None, "inside")


# ---- the node -------------------------------------------------------------------------------------------------------------------------
def test_node_returns_what_the_module_returns_on_the_inputs_device():
    image, mask, plate = _video()
    node = grain_nodes.LanPaint_GrainMatch()
    out, = node.match(torch.from_numpy(image), torch.from_numpy(mask), 1.0, "auto", False, 64, 8, 5, 0)
    assert not out.is_cuda and out.dtype == torch.float32
    _same(out.numpy(), ref.match(image, mask, seed=5), "host in, host out")
    on, on_mask = _dev(image), _dev(mask)
    out, = node.match(on, on_mask, 1.5, "medium", True, 255, 3, 9, 2, reference=torch.from_numpy(plate))
    assert out.device == on.device
    assert torch.equal(out, grain.match(on, on_mask, _dev(plate), 1.5, "medium", True, 255, 3, 9, 2))
    _same(out.cpu().numpy(), ref.match(image, mask, plate, 1.5, 1, True, 255, 3, 9, 2), "device in, device out")
    out, = node.match(torch.from_numpy(image[:1]), torch.from_numpy(mask[0]))
    _same(out.numpy(), ref.match(image[:1], mask[:1]), "one frame, a plane for a mask, the defaults")
