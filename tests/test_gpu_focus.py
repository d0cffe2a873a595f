"""The focus form of lp_multiband_blend on the MI355X against its numpy restatement (tests/focus_ref.py): every comparison is bit for
bit -- `out` over every element, and the statistics, both variances, K and the taps read back from the workspace.  The direct entry
calls get a workspace of exactly focus_ws_bytes bytes and an output that hold 0x00 or 0xFF, with guard words behind both.  Shapes:
sides 1, 10, 11 and 12 around the 11 x 11 support, 37 x 41, 40 x 150 and 65 x 33 around the 32 x 32 tile and its halo; C 1..5 (the luma
rule, channels beyond three); B 1 and 3 with one mask or a mask each.  K is forced to 0, 1, 511 and 512: the rule caps K at
512 (16 px^2 in thirty-seconds), so the largest mixed kernel is K = 511 (k 31, t 15); 16 * 32 + 15 cannot occur."""
import ctypes
import functools
import time

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, focus, focus_nodes, multiband
from lanpaint_amd._util import raw_stream
from tests import focus_ref as fref
from tests import focus_scenes as scenes
from tests import multiband_ref
from tests.device import DELAY_MS, DEV, _spin_cycles_per_ms
from tests.helpers import record_launches
from tests.poison import poisoned_empty

pytestmark = pytest.mark.gpu
GUARD = 64                                                             # bytes behind the workspace and behind the output
FORMS = ("left", "frame", "all", "none", "soft", "nan")
SHAPES = [(1, 1), (10, 40), (40, 10), (11, 11), (12, 12), (37, 41), (40, 150), (65, 33)]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


@functools.lru_cache(maxsize=None)
def _images(B, H, W, C):
    """(image1, image2): random grey blocks of 4 x 4 pixels per channel -- an edge every four pixels, so that the small shapes
    reach 64 edge pixels a side -- and the same through a Gaussian of sigma 1.5, off the 8-bit codes.  Values above 1 in image1's
    last channel exercise the clamp of the codes (finite: a NaN under the blur would make the test one of NaN payloads).
    Read-only."""
    rng = np.random.default_rng([B, H, W, C])
    grey = rng.integers(0, 256, (B, -(-H // 4), -(-W // 4), C)).astype(np.float64)
    levels = np.repeat(np.repeat(grey, 4, 1), 4, 2)[:, :H, :W]
    one = scenes.quantised(levels)
    two = np.empty_like(one)
    for b in range(B):
        for c in range(C):
            two[b, :, :, c] = (scenes.gauss(levels[b, :, :, c], 1.5) / 255.0).astype(np.float32)
    one[:, ::7, ::5, -1] += np.float32(1.5)
    one.setflags(write=False)
    two.setflags(write=False)
    return one, two


@functools.lru_cache(maxsize=None)
def _mask(Bm, H, W, form):
    rng = np.random.default_rng([Bm, H, W, FORMS.index(form)])
    m = np.zeros((Bm, H, W), np.float32)
    for b in range(Bm):
        if form in ("left", "soft", "nan"):                            # touches the top, bottom and left borders
            m[b, :, :max(1, W // 2 - b)] = 1.0
        elif form == "frame":                                          # touches every border, known in the middle
            m[b] = 1.0
            m[b, H // 3:max(H // 3 + 1, 2 * H // 3), W // 3:max(W // 3 + 1, 2 * W // 3 - b)] = 0.0
        elif form == "all":
            m[b] = 1.0
    if form == "soft":                                                 # soft values on both sides of 0.5, above 1 and below 0
        m = (m * np.float32(0.75) + rng.random((Bm, H, W), dtype=np.float32) * np.float32(0.5) - np.float32(0.125)).astype(np.float32)
        m[:, :, W // 2 + 2:] = 0.0
    if form == "nan":                                                  # a NaN is not masked and has no weight
        m[rng.random((Bm, H, W)) < 0.003] = np.nan
        m[:, H // 2, W // 4] = np.nan
    m.setflags(write=False)
    return m


def _cases():
    """(H, W, C, B, Bm, edge, ring, strength16, per_frame, form): every shape with every mask form, the parameters cycling so that
    each value meets each shape."""
    out, i = [], 0
    for H, W in SHAPES:
        for form in FORMS:
            B = 3 if i % 3 == 1 else 1
            out.append((H, W, 1 + (i // 6 + i) % 5, B, B if i % 2 else 1, (1, 3, 2, 1, 2, 255, 1)[i % 7], (1, 8, 2)[i % 3],
                        (16, 9, 1, 16, 0)[i % 5], (i // 3) % 2, form))
            i += 1
    return out


CASES = _cases()


def _case_id(c):
    H, W, C, B, Bm, edge, ring, s16, pf, form = c
    return f"{H}x{W}x{C}-B{B}-M{Bm}-e{edge}-r{ring}-s{s16}-p{pf}-{form}"


@functools.lru_cache(maxsize=None)
def _reference(case):
    """(image1, image2, mask, out, stats, var, K, taps) of a case; computed once, read-only."""
    H, W, C, B, Bm, edge, ring, s16, pf, form = case
    one, two = _images(B, H, W, C)
    mask = _mask(Bm, H, W, form)
    want = fref.match_focus_ref(one, two, mask, edge, ring, s16, pf)
    for a in want:
        a.setflags(write=False)
    return (one, two, mask, *want)


def _direct(hip_lib, one, two, mask, word, poison, stream=None):
    """lp_multiband_blend called directly: `ws` of exactly focus_ws_bytes bytes and `out`, both holding `poison`, each with GUARD
    bytes of the other byte behind it.  `two` None: image2 is image1's tensor.  -> (out, stats, var, K, taps) as numpy."""
    B, H, W, C = one.shape
    t1, mt = torch.from_numpy(one).to(DEV), torch.from_numpy(mask).to(DEV)
    t2 = t1 if two is None else torch.from_numpy(two).to(DEV)
    at = _cabi.focus_ws_layout(B, H, W, C)
    ws_bytes, out_bytes = at["bytes"], one.size * 4
    assert ws_bytes % 16 == 0 and hip_lib.lp_multiband_ws_bytes(B, H, W, C, word) == ws_bytes
    ws = torch.full((ws_bytes + GUARD,), poison, dtype=torch.uint8, device=DEV)
    out = torch.full((out_bytes + GUARD,), poison, dtype=torch.uint8, device=DEV)
    ws[ws_bytes:] = poison ^ 0xFF
    out[out_bytes:] = poison ^ 0xFF
    d = _cabi.LpMultibandDesc(B, H, W, C, mask.shape[0], word, t1.data_ptr(), t2.data_ptr(), mt.data_ptr(), out.data_ptr(),
                              ws.data_ptr(), ws_bytes)
    assert hip_lib.lp_multiband_blend(ctypes.byref(d), raw_stream(DEV) if stream is None else stream) == _cabi.LP_OK
    torch.cuda.synchronize()
    assert (ws[ws_bytes:] == poison ^ 0xFF).all() and (out[out_bytes:] == poison ^ 0xFF).all(), "a guard word was written"
    host = ws[:at["plane"]].cpu().numpy()
    part = lambda name, n, dtype: host[at[name]:at[name] + n].view(dtype)      # noqa: E731
    return (out[:out_bytes].cpu().numpy().view(np.float32).reshape(one.shape), part("stats", B * 48, np.int64).reshape(B, 2, 3),
            part("var", B * 16, np.float64).reshape(B, 2), part("K", B * 4, np.int32), part("taps", B * 67 * 4, np.float32).reshape(B, 67))


def _check(got, want, what):
    """(out, stats, var, K, taps) against the restatement's, every one bit for bit"""
    for name, g, w in zip(("out", "stats", "var", "K", "taps"), got, want):
        if g is None:
            continue
        bad = _bits(g) != _bits(w)
        assert not bad.any(), (what, name, int(bad.sum()), np.argwhere(bad)[:4].tolist(), g[bad][:4].tolist(), w[bad][:4].tolist())


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_the_entry_gives_the_restatements_bits_and_figures(case, hip_lib):
    H, W, C, B, Bm, edge, ring, s16, pf, form = case
    one, two, mask, *want = _reference(case)
    poison = 0xFF if CASES.index(case) % 2 else 0x00
    got = _direct(hip_lib, one, two, mask, _cabi.LP_MULTIBAND_FOCUS(edge, ring, s16, pf), poison)
    _check(got, want, (_case_id(case), hex(poison)))
    m0 = np.broadcast_to(fref.weight0(mask) == 0, one.shape[:3])
    assert (_bits(got[0])[m0] == _bits(one)[m0]).all()                 # where m == 0: image1's bits, the values above 1 too


# the cases both poisons are applied to: several tiles, B 3 with a mask each, a K > 0 and a K = 0
BOTH = [c for c in CASES if (c[0], c[1]) in ((40, 150), (65, 33)) and c[9] in ("left", "soft", "none")] + [c for c in CASES if c[3] == 3 and c[4] == 3][:2]


@pytest.mark.parametrize("case", BOTH, ids=_case_id)
def test_the_entry_reads_no_byte_of_ws_or_out_before_writing_it(case, hip_lib):
    H, W, C, B, Bm, edge, ring, s16, pf, form = case
    one, two, mask, *want = _reference(case)
    for poison in (0x00, 0xFF):
        _check(_direct(hip_lib, one, two, mask, _cabi.LP_MULTIBAND_FOCUS(edge, ring, s16, pf), poison), want, (_case_id(case), hex(poison)))


def test_the_cases_reach_what_they_are_for():
    """Without this a case could pass on an empty job: the forms give both regions, a fit, a blur and the refusals to fit."""
    seen = {"blurred": 0, "measured": 0, "unfit": 0, "pooled": 0}
    for case in CASES:
        H, W, C, B, Bm, edge, ring, s16, pf, form = case
        one, two, mask, out, stats, var, K, taps = _reference(case)
        if form in ("none", "all"):
            assert (K == 0).all() and (stats[:, 0 if form == "all" else 1] == 0).all()
        if min(H, W) < 11:
            assert (stats == 0).all() and (_bits(out) == _bits(one)).all()
        seen["measured"] += int((stats[:, :, 0] >= 64).all())
        seen["unfit"] += int((var == fref.NO_FIT).any())
        seen["blurred"] += int((K > 0).any() and (_bits(out) != _bits(one)).any())
        seen["pooled"] += int(not pf and B == 3 and (K > 0).any())
    assert seen["blurred"] >= 6 and seen["measured"] >= 8 and seen["unfit"] >= 12 and seen["pooled"] >= 1, seen
    assert {c[2] for c in CASES} == {1, 2, 3, 4, 5} and {c[5] for c in CASES} >= {1, 255} and {c[6] for c in CASES} >= {1, 8}
    assert {c[7] for c in CASES} >= {0, 1, 16} and {c[8] for c in CASES} == {0, 1} and {(c[3], c[4]) for c in CASES} == {(1, 1), (3, 1), (3, 3)}


# ---- K at its ends ----------------------------------------------------------------------------------------------------------------------
# (sigma of the stripes' blur outside the mask, the bright grey, strength16, channels) -> the K the restatement fits
FORCED = {0: (0.0, 215.0, 16, 1), 1: (0.56, 215.0, 1, 3), 511: (4.004, 180.0, 16, 4), 512: (4.03, 215.0, 16, 1)}


@functools.lru_cache(maxsize=None)
def _forced(K):
    sigma, hi, s16, C = FORCED[K]
    one, two, mask = scenes.stripes(sigma, channels=C, hi=hi)
    return (one, two, mask, s16, *fref.match_focus_ref(one, two, mask, 1, 2, s16, 0))


@pytest.mark.parametrize("K", sorted(FORCED))
def test_k_at_zero_one_the_largest_mixture_and_the_cap(K, hip_lib):
    one, two, mask, s16, *want = _forced(K)
    assert want[3][0] == K                                             # checked on the CPU: the scene gives this K
    k, t = K >> 4, K & 15
    assert np.count_nonzero(want[4][0]) == 2 * (k + (1 if t else 0)) + 1
    got = _direct(hip_lib, one, None if K == 0 else two, mask, _cabi.LP_MULTIBAND_FOCUS(1, 2, s16, 0), 0xFF)
    _check(got, want, K)
    changed = _bits(got[0]) != _bits(one)
    assert changed.any() == (K > 0) and not changed[0][~(mask[0] > 0)].any()


# ---- the wrapper ------------------------------------------------------------------------------------------------------------------------
WRAP = (40, 150, 3, 3, 3, 1, 2, 16, 1, "left")                         # B 3 with a mask each, per frame; five tiles a row


def _wrap(one, two, mask, case, call=focus.match_focus, **more):
    edge, ring, s16, pf = case[5:9]
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
    return call(dev(one), dev(mask), dev(two), strength=s16 / 16, edge=edge, ring=ring, per_frame=bool(pf), **more)


def test_the_wrapper_the_report_and_the_mask_forms(monkeypatch):
    one, two, mask, *want = _reference(WRAP)
    assert (want[3] > 0).all()
    names = record_launches(monkeypatch, focus)
    got = _wrap(one, two, mask, WRAP)
    assert names == ["lp_multiband_blend"]                             # one entry call for the whole batch
    assert got.is_cuda and got.dtype == torch.float32
    _check((got.cpu().numpy(), None, None, None, None), want, "a mask each")
    rep = _wrap(one, two, mask, WRAP, call=focus.focus_report)
    assert all(rep[k].is_cuda for k in rep) and rep["var_ring"].dtype == torch.float64 and rep["K"].dtype == torch.int32
    var = torch.stack([rep["var_ring"], rep["var_inside"]], 1).cpu().numpy()
    _check((rep["image"].cpu().numpy(), None, var, rep["K"].cpu().numpy(), None), want, "the report")
    shared = _wrap(one, two, mask[1:2], WRAP).cpu().numpy()            # mask_batch 1: every image under image 1's mask
    assert (_bits(shared) == _bits(fref.match_focus_ref(one, two, mask[1:2], *WRAP[5:9])[0])).all()
    assert (_bits(_wrap(one, two, mask[1], WRAP).cpu().numpy()) == _bits(shared)).all()      # [H, W]
    own = _wrap(one, None, mask, WRAP).cpu().numpy()                   # no reference: the ring is read on the image itself
    assert (_bits(own) == _bits(fref.match_focus_ref(one, one, mask, *WRAP[5:9])[0])).all()


def test_a_frame_gives_the_same_bits_alone_in_a_batch_and_in_chunks(monkeypatch):
    one, two, mask, *want = _reference(WRAP)
    for b in range(3):
        alone = _wrap(one[b:b + 1], two[b:b + 1], mask[b:b + 1], WRAP).cpu().numpy()
        assert (_bits(alone[0]) == _bits(want[0][b])).all(), b
    names = record_launches(monkeypatch, focus)
    H, W, C = WRAP[:3]
    monkeypatch.setattr(focus, "WS_CAP_BYTES", _cabi.focus_ws_bytes(1, H, W, C) + 8)
    rep = _wrap(one, two, mask, WRAP, call=focus.focus_report)
    assert names == ["lp_multiband_blend"] * 3                         # one image a chunk, one entry call per chunk
    var = torch.stack([rep["var_ring"], rep["var_inside"]], 1).cpu().numpy()
    _check((rep["image"].cpu().numpy(), None, var, rep["K"].cpu().numpy(), None), want, "chunked")
    shared = _wrap(one, two, mask[:1], WRAP).cpu().numpy()             # chunks under one mask plane
    assert (_bits(shared) == _bits(fref.match_focus_ref(one, two, mask[:1], *WRAP[5:9])[0])).all()
    # the pooled form measures the clip as one: it is refused rather than measured in parts
    pooled = WRAP[:8] + (0,) + WRAP[9:]
    with pytest.raises(ValueError, match="per_frame=True"):
        _wrap(one, two, mask, pooled)
    monkeypatch.setattr(focus, "WS_CAP_BYTES", 1 << 30)
    got = _wrap(one, two, mask, pooled).cpu().numpy()
    want_pooled = fref.match_focus_ref(one, two, mask, *pooled[5:9])
    assert (_bits(got) == _bits(want_pooled[0])).all() and len(set(want_pooled[3].tolist())) == 1
    assert set(want_pooled[3].tolist()) != set(want[3].tolist())       # pooling is no no-op on this batch


def test_views_half_precision_and_the_node():
    one, two, mask, *want = _reference(WRAP)
    wide = np.ascontiguousarray(np.repeat(one, 2, 1))
    it = torch.from_numpy(wide).to(DEV)
    got = focus.match_focus(it[:, ::2], torch.from_numpy(mask).to(DEV), torch.from_numpy(two).to(DEV), edge=1, per_frame=True)
    assert (_bits(got.cpu().numpy()) == _bits(want[0])).all()          # not contiguous
    half = torch.from_numpy(two).to(DEV).to(torch.float16)
    got = focus.match_focus(half, torch.from_numpy(mask).to(DEV), edge=1, per_frame=True)
    h32 = half.float().cpu().numpy()
    assert got.dtype == torch.float32 and (_bits(got.cpu().numpy()) == _bits(fref.match_focus_ref(h32, h32, mask, 1, 2, 16, 1)[0])).all()
    with pytest.raises(ValueError):
        focus.match_focus(it, torch.from_numpy(mask).to(DEV))          # the mask's height is not the image's
    out, = focus_nodes.LanPaint_FocusMatch().match(torch.from_numpy(one.copy()), torch.from_numpy(mask.copy()), 1.0, 1, 2, True,
                                                   reference=torch.from_numpy(two.copy()))
    assert not out.is_cuda and out.dtype == torch.float32 and (_bits(out.numpy()) == _bits(want[0])).all()


def test_blend_multiband_is_what_it_was():
    """levels >= 0 went through the entry's new branch: levels 0 and 5 equal the blend's own restatement as before."""
    one, two = _images(2, 40, 150, 3)
    one = np.clip(one, 0, 1)
    mask = _mask(1, 40, 150, "soft")
    for levels in (0, 5):
        got = multiband.blend_multiband(torch.from_numpy(one).to(DEV), torch.from_numpy(two).to(DEV), torch.from_numpy(mask).to(DEV), levels)
        assert (_bits(got.cpu().numpy()) == _bits(multiband_ref.blend_ref(one, two, mask, levels))).all(), levels


# ---- off the null stream, behind a delay; the launch record -----------------------------------------------------------------------------
def test_the_wrapper_on_a_held_back_side_stream_reads_nothing_back(monkeypatch):
    """As tests/test_gpu_patch_fill.py has it: made on a side stream that is still busy with a delay, the call returns before the
    delay is done (no device -> host read, no synchronisation), leaves nothing on the null stream, makes one lp_multiband_blend call,
    and every launch waits behind the 0xFF fills of its buffers, or the bits differ."""
    one, two, mask, *want = _reference(WRAP)
    t1, t2, mt = (torch.from_numpy(a).to(DEV) for a in (one, two, mask))
    run = lambda: focus.focus_report(t1, mt, t2, edge=1, per_frame=True)      # noqa: E731
    per_ms = _spin_cycles_per_ms()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        run()                                                          # loads the kernels, fills this stream's allocator pool
        side.synchronize()
        reads = []
        for method in ("cpu", "item", "tolist", "numpy"):
            def counted(self, *args, _real=getattr(torch.Tensor, method), _name=method, **kwargs):
                if self.is_cuda:
                    reads.append(_name)
                return _real(self, *args, **kwargs)
            monkeypatch.setattr(torch.Tensor, method, counted)
        names = record_launches(monkeypatch, focus)
        filled = poisoned_empty(monkeypatch, 0xFF)
        done = torch.cuda.Event()
        torch.cuda._sleep(int(per_ms * DELAY_MS))
        done.record(side)
        start = time.perf_counter()
        rep = run()
        held = not done.query()
        idle = torch.cuda.default_stream().query()
        call_ms = (time.perf_counter() - start) * 1e3
        print(f"FOCUS_SIDE call behind the delay {call_ms:.2f} ms of host time; delay {DELAY_MS} ms")
        assert held, f"returned after {call_ms:.2f} ms with the {DELAY_MS} ms delay done: it waited for the device"
        assert idle, "work was left on the null stream"
        assert names == ["lp_multiband_blend"] and reads == [] and len(filled) >= 2          # the workspace and the output
        side.synchronize()
    monkeypatch.undo()
    var = torch.stack([rep["var_ring"], rep["var_inside"]], 1).cpu().numpy()
    _check((rep["image"].cpu().numpy(), None, var, rep["K"].cpu().numpy(), None), want, "behind the delay")
