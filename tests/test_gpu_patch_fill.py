"""The patch form of lp_mask_fill on the MI355X against its numpy restatement (tests/patch_fill_ref.py): every comparison is bit
for bit over every element, and the level-0 field read back from the workspace is compared over the targets too.  The direct
entry calls get a workspace of exactly fill_patch_ws_bytes bytes and an output that hold 0x00 or 0xFF, with guard words behind
both.  Shapes: 1 x 1, single rows and columns, 5 x 5 (one possible source centre at r 2), sides around one and two 16 x 16 tiles
and around the 32 x 32 tile of the push-pull launches; B 1 and 3."""
import ctypes
import functools
import time

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, fill, fill_patch_nodes
from lanpaint_amd._util import raw_stream
from tests import patch_fill_ref as pref
from tests.compare import _raw_bits as _bits
from tests.device import DELAY_MS, DEV, _spin_cycles_per_ms
from tests.helpers import record_launches
from tests.poison import poisoned_empty

pytestmark = pytest.mark.gpu
GUARD = 64                                                             # bytes behind the workspace and behind the output
FORMS = ("centre", "borders", "speckle30", "speckle2", "known", "masked", "corner", "nan", "half")
SMALL_SHAPES = [(1, 1, 3), (1, 7, 1), (7, 1, 4), (5, 5, 3)]
LARGE_SHAPES = [(31, 33, 3), (33, 65, 4), (64, 96, 1), (65, 129, 2)]


@functools.lru_cache(maxsize=None)
def _image(B, H, W, C, kind):
    """"noise": random values; "tile": a random 3 x 4 tile of exact codes repeated, so that equal distances are common and the
    key's (s_y, s_x) decides.  Read-only."""
    rng = np.random.default_rng([B, H, W, C, len(kind)])
    if kind == "noise":
        img = (np.float32(0.02) + np.float32(0.96) * rng.random((B, H, W, C), dtype=np.float32)).astype(np.float32)
    else:
        tile = (rng.integers(13, 243, (B, 3, 4, C)).astype(np.float32) / np.float32(255)).astype(np.float32)
        img = np.tile(tile, (1, -(-H // 3), -(-W // 4), 1))[:, :H, :W]
    img = np.ascontiguousarray(img)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _mask(Bm, H, W, form):
    rng = np.random.default_rng([Bm, H, W, FORMS.index(form)])
    m = np.zeros((Bm, H, W), np.float32)
    for b in range(Bm):
        if form in ("centre", "nan", "half"):
            y0, x0 = (H - 1) // 3 + (b if H > 8 else 0), (W - 1) // 3
            m[b, y0:max(y0 + 1, 2 * H // 3), x0:max(x0 + 1, 2 * W // 3)] = 1.0
        elif form == "borders":
            m[b, :max(1, H // 2 - b), :max(1, W // 3)] = 1.0
        elif form == "speckle30":
            m[b] = rng.random((H, W)) < 0.3
        elif form == "speckle2":
            m[b] = rng.random((H, W)) < 0.02
            m[b, H // 2, W // 2] = 1.0
        elif form == "masked":
            m[b] = 1.0
        elif form == "corner":
            m[b] = 1.0
            m[b, H - 1, 0] = 0.0
    if form == "nan":                                                  # a NaN is not masked: inside the hole it is a known pixel
        m[rng.random((Bm, H, W)) < 0.05] = np.nan
    if form == "half":                                                 # exactly 0.5 is known, the next float above is masked
        m = np.where(m > 0, np.nextafter(np.float32(0.5), np.float32(1)), np.float32(0.5)).astype(np.float32)
    m.setflags(write=False)
    return m


def _cases():
    """(H, W, C, B, Bm, r, levels, iters, seed, form, kind): every large shape with every mask form, the parameters cycling so that
    each of r in {1, 2, 4}, levels in {1, 2, 3}, iters in {1, 3} and both seeds meets each shape; the small shapes with the
    forms that differ on them."""
    out, i = [], 0
    for H, W, C in LARGE_SHAPES:
        for form in FORMS:
            B = 3 if i % 4 == 1 else 1
            out.append((H, W, C, B, B if i % 8 == 1 else 1, (1, 2, 4)[i % 3], (1, 2, 3)[(i // 3) % 3], (1, 3)[(i // 2) % 2],
                        (0, 40001)[i % 2], form, ("noise", "tile")[(i // 2) % 2]))
            i += 1
    for H, W, C in SMALL_SHAPES:
        for form in ("centre", "known", "masked", "corner"):
            out.append((H, W, C, 3 if i % 2 else 1, 1, (1, 2, 4)[i % 3], (1, 2, 3)[(i // 3) % 3], (1, 3)[i % 2], (0, 40001)[(i // 2) % 2],
                        form, "noise"))
            i += 1
    out.append((5, 5, 3, 1, 1, 1, 2, 3, 0, "corner", "tile"))          # r 1 on 5 x 5: nine centres
    out.append((5, 5, 3, 3, 3, 2, 1, 3, 1, "known", "noise"))          # r 2 on 5 x 5: the one centre, and no target
    return out


CASES = _cases()


def _case_id(c):
    H, W, C, B, Bm, r, L, iters, seed, form, kind = c
    return f"{H}x{W}x{C}-B{B}-M{Bm}-r{r}-L{L}-i{iters}-s{seed}-{form}-{kind}"


@functools.lru_cache(maxsize=None)
def _reference(case):
    """(image, mask, out, field, target) of a case; computed once, read-only."""
    H, W, C, B, Bm, r, L, iters, seed, form, kind = case
    img, mask = _image(B, H, W, C, kind), _mask(Bm, H, W, form)
    want = pref.fill_ref_patch(img, mask, r, L, iters, seed)
    for a in want:
        a.setflags(write=False)
    return (img, mask, *want)


def _direct(hip_lib, img, mask, r, L, iters, seed, poison, stream=None):
    """lp_mask_fill called directly: `ws` of exactly fill_patch_ws_bytes bytes and `out`, both holding `poison`, each with GUARD
    bytes of the other byte behind it.  -> (out [B, H, W, C] numpy, the level-0 field [B, H, W] int32)."""
    B, H, W, C = img.shape
    it, mt = torch.from_numpy(img).to(DEV), torch.from_numpy(mask).to(DEV)
    ws_bytes = _cabi.fill_patch_ws_bytes(B, H, W, C, L)
    out_bytes = img.size * 4
    assert ws_bytes % 16 == 0
    ws = torch.full((ws_bytes + GUARD,), poison, dtype=torch.uint8, device=DEV)
    out = torch.full((out_bytes + GUARD,), poison, dtype=torch.uint8, device=DEV)
    ws[ws_bytes:] = poison ^ 0xFF
    out[out_bytes:] = poison ^ 0xFF
    d = _cabi.LpFillDesc(B, H, W, C, mask.shape[0], _cabi.LP_FILL_PATCH(r, L, iters, seed), it.data_ptr(), mt.data_ptr(), out.data_ptr(),
                         ws.data_ptr(), ws_bytes)
    assert hip_lib.lp_mask_fill(ctypes.byref(d), raw_stream(DEV) if stream is None else stream) == _cabi.LP_OK
    torch.cuda.synchronize()
    assert (ws[ws_bytes:] == poison ^ 0xFF).all() and (out[out_bytes:] == poison ^ 0xFF).all(), "a guard word was written"
    at = _cabi.fill_patch_ws_layout(B, H, W, C, L)[0]["nnf"]
    field = ws[at:at + 4 * B * H * W].cpu().numpy().view(np.int32).reshape(B, H, W)
    return out[:out_bytes].cpu().numpy().view(np.float32).reshape(img.shape), field


def _check(got, field, case, what):
    img, mask, want, want_field, target = _reference(case)
    bad = _bits(got) != _bits(want)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    if field is not None:
        bad = (field != want_field) & target
        assert not bad.any(), (what, "field", int(bad.sum()), np.argwhere(bad)[:4].tolist())
        assert (field[~target] == -1).all(), (what, "field outside the targets")
    known = np.broadcast_to(~(mask > 0.5), img.shape[:3])
    assert (_bits(got)[known] == _bits(img)[known]).all(), what


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_the_entry_gives_the_restatements_bits_and_field(case, hip_lib):
    H, W, C, B, Bm, r, L, iters, seed, form, kind = case
    img, mask = _reference(case)[:2]
    poison = 0xFF if CASES.index(case) % 2 else 0x00
    got, field = _direct(hip_lib, img, mask, r, L, iters, seed, poison)
    _check(got, field, case, (_case_id(case), hex(poison)))


# the cases the two poisons are both applied to: several tiles and levels, B 3 with a mask each, the fallback, no target at all
BOTH = [c for c in CASES if (c[0], c[1]) == (65, 129) and c[9] in ("centre", "speckle30", "known")] + \
       [c for c in CASES if c[3] == 3 and c[4] == 3][:2]


@pytest.mark.parametrize("case", BOTH, ids=_case_id)
def test_the_entry_reads_no_byte_of_ws_or_out_before_writing_it(case, hip_lib):
    H, W, C, B, Bm, r, L, iters, seed, form, kind = case
    img, mask = _reference(case)[:2]
    fields = []
    for poison in (0x00, 0xFF):
        got, field = _direct(hip_lib, img, mask, r, L, iters, seed, poison)
        _check(got, field, case, (_case_id(case), hex(poison)))
        fields.append(field)
    assert (fields[0] == fields[1]).all()


def test_the_cases_reach_what_they_are_for():
    """Without this a case could pass on an empty job: the forms give targets, sources, votes and the fallback as intended."""
    seen = {"filled": 0, "fallback": 0, "partial": 0}
    for case in CASES:
        H, W, C, B, Bm, r, L, iters, seed, form, kind = case
        if (H, W, C) not in LARGE_SHAPES:
            continue
        img, mask, want, field, target = _reference(case)
        hole = np.broadcast_to(mask > 0.5, target.shape)
        if form == "known":
            assert not target.any() and (_bits(want) == _bits(img)).all()
        elif form in ("masked", "corner"):
            assert target.all() and (field == -1).all()                # no source: the push-pull result
            seen["fallback"] += 1
        elif form in ("centre", "borders", "nan", "half"):
            assert hole.any() and not hole.all()
            seen["filled"] += int((field[target] >= 0).all())
        elif form == "speckle30" and (field == -1).all():
            seen["fallback"] += 1
        else:
            seen["partial"] += int((field[target] >= 0).any())
    # of the 16 cases with a compact hole at least half end with an entry at every target (one round can leave a target without);
    # the 8 without a known patch and some speckles fall back; the sparse speckles fill in part
    assert seen["filled"] >= 8 and seen["fallback"] >= 8 and seen["partial"] >= 3, seen
    assert {c[5] for c in CASES} == {1, 2, 4} and {c[6] for c in CASES} == {1, 2, 3} and {c[7] for c in CASES} == {1, 3}
    assert {c[8] for c in CASES} == {0, 1, 40001} and {c[3] for c in CASES} == {1, 3} and {c[9] for c in CASES} == set(FORMS)


# ---- the wrapper ------------------------------------------------------------------------------------------------------------------------
WRAP = (33, 65, 4, 3, 3, 2, 2, 3, 5, "centre", "noise")               # B 3 with a mask each; two levels; three tiles a row


def _wrap(img, mask, case, **more):
    r, L, iters, seed = case[5:9]
    return fill.fill_masked_patch(torch.from_numpy(np.ascontiguousarray(img)).to(DEV), torch.from_numpy(np.ascontiguousarray(mask)).to(DEV),
                                  radius=r, levels=L, iters=iters, seed=seed, **more)


def test_the_wrapper_one_mask_for_all_and_a_mask_each(monkeypatch):
    img, mask, want = _reference(WRAP)[:3]
    names = record_launches(monkeypatch, fill)
    got = _wrap(img, mask, WRAP)
    assert names == ["lp_mask_fill"]                                   # one entry call for the whole batch
    assert got.is_cuda and got.dtype == torch.float32
    _check(got.cpu().numpy(), None, WRAP, "a mask each")
    shared = _wrap(img, mask[1:2], WRAP).cpu().numpy()                 # mask_batch 1: every image under image 1's mask
    one = pref.fill_ref_patch(img, mask[1:2], *WRAP[5:9])[0]
    assert (_bits(shared) == _bits(one)).all() and (_bits(shared[1]) == _bits(want[1])).all()
    plain = _wrap(img, mask[1], WRAP).cpu().numpy()                    # [H, W]
    assert (_bits(plain) == _bits(shared)).all()


def test_a_frame_gives_the_same_bits_alone_in_a_batch_and_in_chunks(monkeypatch):
    img, mask, want = _reference(WRAP)[:3]
    for b in range(3):
        alone = _wrap(img[b:b + 1], mask[b:b + 1], WRAP).cpu().numpy()
        assert (_bits(alone[0]) == _bits(want[b])).all(), b
    names = record_launches(monkeypatch, fill)
    H, W, C = WRAP[:3]
    monkeypatch.setattr(fill, "WS_CAP_BYTES", _cabi.fill_patch_ws_bytes(1, H, W, C, WRAP[6]) + 8)
    chunked = _wrap(img, mask, WRAP).cpu().numpy()
    assert names == ["lp_mask_fill"] * 3                               # one image a chunk, one entry call per chunk
    assert (_bits(chunked) == _bits(want)).all()
    shared = _wrap(img, mask[:1], WRAP).cpu().numpy()                  # chunks under one mask plane
    assert (_bits(shared) == _bits(pref.fill_ref_patch(img, mask[:1], *WRAP[5:9])[0])).all()


def test_nan_under_the_mask_changes_nothing_and_two_calls_agree():
    img, mask, want = _reference(WRAP)[:3]
    hole = np.broadcast_to((mask > 0.5)[..., None], img.shape)
    poisoned = np.where(hole, np.float32(np.nan), img).astype(np.float32)
    first, second = _wrap(poisoned, mask, WRAP).cpu().numpy(), _wrap(img, mask, WRAP).cpu().numpy()
    assert (_bits(first) == _bits(want)).all() and (_bits(second) == _bits(want)).all()


def test_auto_levels_views_and_half_precision():
    img = _image(2, 66, 130, 3, "tile")
    mask = _mask(1, 33, 130, "centre")
    it = torch.from_numpy(img).to(DEV)
    got = fill.fill_masked_patch(it[:, ::2], torch.from_numpy(mask[0]).to(DEV), radius=1)          # not contiguous; AUTO; mask [H, W]
    L = fill.patch_levels(33, 130, 1)
    assert L == 2
    want = pref.fill_ref_patch(np.ascontiguousarray(img[:, ::2]), mask, 1, L, 4, 0)[0]
    assert (_bits(got.cpu().numpy()) == _bits(want)).all()
    half = it[:, :33].to(torch.float16)
    got = fill.fill_masked_patch(half, torch.from_numpy(mask).to(DEV), radius=1, levels=1, iters=2, seed=9)
    assert got.dtype == torch.float32
    assert (_bits(got.cpu().numpy()) == _bits(pref.fill_ref_patch(half.float().cpu().numpy(), mask, 1, 1, 2, 9)[0])).all()
    with pytest.raises(ValueError):
        fill.fill_masked_patch(it, torch.from_numpy(mask).to(DEV))     # the mask's height is not the image's


def test_the_node_runs_end_to_end_from_host_tensors():
    img, mask, want = _reference(WRAP)[:3]
    r, L, iters, seed = WRAP[5:9]
    out, = fill_patch_nodes.LanPaint_MaskFillPatch().fill(torch.from_numpy(img.copy()), torch.from_numpy(mask.copy()), r, L, iters, seed)
    assert not out.is_cuda and out.dtype == torch.float32
    assert (_bits(out.numpy()) == _bits(want)).all()


# ---- off the null stream, behind a delay; the launch record -----------------------------------------------------------------------------------
def test_the_wrapper_on_a_held_back_side_stream_reads_nothing_back(monkeypatch):
    """As tests/test_gpu_image_scratch.py has it for fill_masked: made on a side stream that is still busy with a delay, the call
    returns before the delay is done (no device -> host read, no synchronisation), leaves nothing on the null stream, makes one
    lp_mask_fill call per chunk, and every launch waits behind the 0xFF fills of its buffers, or the bits differ."""
    img, mask, want = _reference(WRAP)[:3]
    it, mt = torch.from_numpy(img).to(DEV), torch.from_numpy(mask).to(DEV)
    r, L, iters, seed = WRAP[5:9]
    run = lambda: fill.fill_masked_patch(it, mt, radius=r, levels=L, iters=iters, seed=seed)       # noqa: E731
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
        names = record_launches(monkeypatch, fill)
        filled = poisoned_empty(monkeypatch, 0xFF)
        done = torch.cuda.Event()
        torch.cuda._sleep(int(per_ms * DELAY_MS))
        done.record(side)
        start = time.perf_counter()
        got = run()
        held = not done.query()
        idle = torch.cuda.default_stream().query()
        call_ms = (time.perf_counter() - start) * 1e3
        print(f"PATCH_SIDE call behind the delay {call_ms:.2f} ms of host time; delay {DELAY_MS} ms")
        assert held, f"returned after {call_ms:.2f} ms with the {DELAY_MS} ms delay done: it waited for the device"
        assert idle, "work was left on the null stream"
        assert names == ["lp_mask_fill"] and reads == [] and len(filled) >= 2          # the workspace and the output
        side.synchronize()
    assert (_bits(got.cpu().numpy()) == _bits(want)).all()
