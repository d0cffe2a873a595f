"""The mask refine on the MI355X (lanpaint_amd.refine, csrc/refine_kernel.hip) against the numpy restatement tests/refine_ref.py.
The rule fixes every value and the order of every floating-point operation, so the device must give the restatement's bits,
whatever tile, chunk or halo a launch uses: every comparison covers every element and has no tolerance."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, refine, refine_nodes, videomask
from lanpaint_amd._util import raw_stream
from tests import refine_ref as ref
from tests.compare import _raw_bits as _bits
from tests.device import DEV
from tests.image_inputs import _guide, _refine_blobs as _blobs, _rng, _soft

pytestmark = pytest.mark.gpu
# (H, W, C, B, mask_batch, r): degenerate axes, windows wider than the image, several tiles and chunks, a grey guide, a fourth
# channel that is not read, the largest radius; then one under, at and one over the tile sides (32 wide, 32 tall in the first
# launch, 64 tall in the second) and the 16-row chunk
SHAPES = [(1, 1, 3, 1, 1, 1), (1, 7, 3, 1, 1, 64), (7, 1, 1, 2, 1, 3), (5, 9, 4, 1, 1, 8), (33, 65, 3, 2, 2, 1),
          (64, 64, 3, 1, 1, 16), (70, 150, 3, 3, 1, 8), (97, 203, 1, 2, 2, 32), (130, 131, 3, 1, 1, 64), (40, 260, 3, 7, 7, 5),
          (31, 33, 3, 1, 1, 2), (32, 32, 3, 2, 2, 3), (33, 31, 1, 1, 1, 4), (63, 32, 3, 1, 1, 2), (64, 31, 3, 1, 1, 9),
          (65, 33, 3, 1, 1, 7), (15, 17, 3, 1, 1, 1), (16, 16, 3, 1, 1, 8), (17, 15, 3, 1, 1, 24)]
EPS = (1e-6, 1e-3, 1.0)


def _single(Bm, H, W):
    m = np.zeros((Bm, H, W), dtype=np.float32)
    m[:, H // 2, W // 3] = 1.0
    return m


def _boundaries(Bm, H, W, seed=3):
    """k / 255, (k + 0.5) / 255 and their float neighbours: where a code changes."""
    rng = _rng(Bm, H, W, seed)
    k = rng.integers(0, 256, (Bm, H, W))
    v = ((k + rng.choice([0.0, 0.5], (Bm, H, W))) / 255.0).astype(np.float32)
    step = rng.integers(-1, 2, (Bm, H, W))
    return np.where(step < 0, np.nextafter(v, np.float32(-1)), np.where(step > 0, np.nextafter(v, np.float32(2)), v)).astype(np.float32)


def _wild(Bm, H, W, seed=4):
    """NaN, infinities and values outside [0, 1]."""
    rng = _rng(Bm, H, W, seed)
    m = (3.0 * rng.random((Bm, H, W)) - 1.0).astype(np.float32)
    pick = rng.random((Bm, H, W))
    m[pick < 0.15] = np.nan
    m[(pick >= 0.15) & (pick < 0.2)] = np.inf
    m[(pick >= 0.2) & (pick < 0.25)] = -np.inf
    return m


FORMS = {"soft": _soft, "blobs": _blobs, "all 0": lambda *s: np.zeros(s, np.float32), "all 1": lambda *s: np.ones(s, np.float32),
         "single": _single, "boundaries": _boundaries, "wild": _wild}


def _refine(guide, mask, r, eps, **kw):
    g, m = torch.from_numpy(guide).to(DEV), torch.from_numpy(mask).to(DEV)
    return refine.refine_mask(g, m, radius=r, eps=eps, **kw).cpu().numpy()


def _check(guide, mask, r, eps, what):
    got = _refine(guide, mask, r, eps)
    want = ref.refine_ref(guide, mask, r, eps)
    assert got.dtype == np.float32 and got.shape == want.shape, what
    bad = _bits(got) != _bits(want)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), float(np.abs(got - want).max()))
    return got


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_refine_equals_the_restatement_bit_for_bit(shape):
    H, W, C, B, Bm, r = shape
    guide = _guide(B, H, W, C)
    for name in ("soft", "blobs"):
        mask = FORMS[name](Bm, H, W)
        for eps in EPS:
            got = _check(guide, mask, r, eps, (shape, name, eps))
            if name == "soft" and eps == 1e-3:
                assert (_bits(_refine(guide, mask, r, eps)) == _bits(got)).all(), (shape, "two calls")


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("shape", [(70, 150, 3, 2, 2, 8), (40, 50, 1, 2, 1, 3)], ids=lambda s: "x".join(map(str, s)))
def test_every_mask_form_equals_the_restatement(shape, form):
    H, W, C, B, Bm, r = shape
    guide = _guide(B, H, W, C, 5)
    if form in ("boundaries", "wild"):                               # the guide's codes take the same path
        guide[0] = FORMS[form](C, H, W, 6).transpose(1, 2, 0)
    mask = FORMS[form](Bm, H, W)
    for eps in EPS:
        got = _check(guide, mask, r, eps, (shape, form, eps))
        if form == "all 0":
            assert (_bits(got) == 0).all()
        if form == "all 1":
            assert (_bits(got) == _bits(np.float32(1.0))).all()


def test_the_largest_sums_do_not_overflow():
    H, W, r = 130, 131, 64
    ones = np.ones((1, H, W, 3), np.float32)
    got = _check(ones, np.ones((1, H, W), np.float32), r, 1e-3, "all 1.0")
    assert (_bits(got) == _bits(np.float32(1.0))).all()
    binary = (_rng(H, W, 7).random((1, H, W, 3)) < 0.5).astype(np.float32)
    binary[0, 20:110, 10:120] = 1.0                                  # whole windows of code 255 in every plane
    for eps in (1e-6, 1.0):
        _check(binary, np.ascontiguousarray(binary[..., 1]), r, eps, ("codes 0 or 255", eps))


@functools.lru_cache(maxsize=None)
def _reach_case():
    guide = _guide(2, 130, 200, 3, 7)
    mask = np.zeros((2, 130, 200), dtype=np.float32)
    mask[0, 64, 100], mask[1, 0, 0], mask[1, 129, 199] = 1.0, 0.5, 2.0
    return guide, mask


@pytest.mark.parametrize("r", [1, 5, 16, 30])
def test_the_device_output_reaches_no_further_than_2r(r):
    guide, mask = _reach_case()
    yy, xx = np.mgrid[:130, :200]
    far = np.stack([np.maximum(abs(yy - 64), abs(xx - 100)) > 2 * r,
                    np.minimum(np.maximum(yy, xx), np.maximum(129 - yy, 199 - xx)) > 2 * r])
    assert far[0].any() and far[1].any()
    got = _refine(guide, mask, r, 1e-3)
    assert (_bits(got)[far] == 0).all() and (got != 0).any(axis=(1, 2)).all()
    got = _refine(guide, (1.0 - np.clip(mask, 0, 1)).astype(np.float32), r, 1e-3)
    assert (_bits(got)[far] == _bits(np.float32(1.0))).all() and (got != 1).any(axis=(1, 2)).all()


@pytest.mark.parametrize("guard", [64, 3], ids=["aligned", "off 16 bytes"])
@pytest.mark.parametrize("shape", [(70, 150, 3, 8), (65, 33, 1, 20), (130, 131, 4, 64)], ids=lambda s: "x".join(map(str, s)))
def test_entry_does_not_read_its_workspace_before_writing_it_and_stays_inside_out(shape, guard, hip_lib):
    H, W, C, r = shape
    B, eps = 2, 1e-3
    guide, mask = _guide(B, H, W, C, 3), _soft(B, H, W, 17)
    gt, mt = torch.from_numpy(guide).to(DEV), torch.from_numpy(mask).to(DEV)
    ws_bytes = hip_lib.lp_refine_ws_bytes(B, H, W, C, r)
    assert ws_bytes == _cabi.refine_ws_bytes(B, H, W, C, r)
    ws = torch.full((ws_bytes // 4 + 64,), float("nan"), dtype=torch.float32, device=DEV)
    n = B * H * W
    buf = torch.full((n + 2 * guard,), float("nan"), dtype=torch.float32, device=DEV)
    out = buf[guard:guard + n]
    d = _cabi.LpRefineDesc(B, H, W, C, B, r, eps, gt.data_ptr(), mt.data_ptr(), out.data_ptr(), ws.data_ptr(), ws_bytes)
    assert hip_lib.lp_mask_refine(ctypes.byref(d), raw_stream(DEV)) == _cabi.LP_OK
    host = buf.cpu().numpy()
    assert np.isnan(host[:guard]).all() and np.isnan(host[guard + n:]).all(), "guard elements overwritten"
    assert np.isnan(ws[ws_bytes // 4:].cpu().numpy()).all(), "written past the workspace"
    got = host[guard:guard + n].reshape(B, H, W)
    assert (_bits(got) == _bits(ref.refine_ref(guide, mask, r, eps))).all()


def test_chunks_give_the_bits_of_one_call(monkeypatch):
    guide, mask = _guide(3, 63, 65, 3, 11), _soft(3, 63, 65, 13)
    whole = _check(guide, mask, 6, 1e-3, "one call")
    per_image = _cabi.refine_ws_bytes(1, 63, 65, 3, 6)
    for images in (1, 2):
        monkeypatch.setattr(refine, "WS_CAP_BYTES", images * per_image + 8)
        assert (_bits(_refine(guide, mask, 6, 1e-3)) == _bits(whole)).all(), images
        assert (_bits(_refine(guide, mask[:1], 6, 1e-3)) == _bits(_check(guide, mask[:1], 6, 1e-3, "one mask"))).all(), images
    monkeypatch.setattr(refine, "WS_CAP_BYTES", 1)                  # always at least one image per chunk
    assert (_bits(_refine(guide, mask, 6, 1e-3)) == _bits(whole)).all()


def _drifting_blobs(F, H, W, seed):
    """tests/test_gpu_stabilize.py's blobs: a disc that drifts and jitters, an empty frame and a stray blob in it."""
    rng = _rng(F, H, W, seed)
    yy, xx = np.mgrid[:H, :W]
    m = np.zeros((F, H, W), dtype=np.float32)
    for t in range(F):
        cy, cx = H / 2 + rng.normal(0, 1), W / 3 + 0.7 * t + rng.normal(0, 1)
        m[t] = (yy - cy) ** 2 + (xx - cx) ** 2 <= (min(H, W) / 3 + rng.normal(0, 1)) ** 2
    m[F // 3] = 0.0
    m[F // 2, :2, -3:] = 1.0
    return m


def test_grow_chunks_give_the_bits_of_one_call(monkeypatch):
    """grow_mask hands the EDT no more frames at a time than stay under WS_CAP_BYTES, and chunking changes no bit."""
    F, H, W = 7, 21, 40
    mask = _drifting_blobs(F, H, W, 15)
    t = torch.from_numpy(mask).to(DEV)
    seen, edt = [], videomask.keyframe_edt

    def recorder(keys):
        seen.append(int(keys.shape[0]))
        return edt(keys)
    monkeypatch.setattr(videomask, "keyframe_edt", recorder)
    per_frame = videomask.EDT_BYTES_PER_PIXEL * H * W
    for grow in (3, -2):
        whole = refine.grow_mask(t, grow).cpu().numpy()
        assert (_bits(whole) == _bits(np.stack([ref.grow_ref(m, grow) for m in mask]))).all(), grow
        for frames, cap in ((1, per_frame + 8), (2, 2 * per_frame + 8), (3, 3 * per_frame + 8), (0, 1)):
            monkeypatch.setattr(refine, "WS_CAP_BYTES", cap)
            del seen[:]
            got = refine.grow_mask(t, grow).cpu().numpy()
            print(f"GROW_CHUNKS grow={grow} cap={cap} calls={seen}")
            assert (_bits(got) == _bits(whole)).all(), (grow, frames)
            assert max(seen) <= max(1, frames) and sum(seen) == F, (grow, frames, seen)
        monkeypatch.setattr(refine, "WS_CAP_BYTES", 1 << 30)


def test_wrapper_takes_views_half_precision_and_a_plain_mask():
    guide, mask = _guide(2, 66, 100, 3, 4), _soft(1, 33, 100, 19)
    gt = torch.from_numpy(guide).to(DEV)
    got = refine.refine_mask(gt[:, ::2], torch.from_numpy(mask[0]).to(DEV), 4, 1e-2).cpu().numpy()                 # mask [H, W]
    assert (_bits(got) == _bits(ref.refine_ref(np.ascontiguousarray(guide[:, ::2]), mask, 4, 1e-2))).all()
    hg = gt[:, :33].to(torch.float16)
    hm = torch.from_numpy(mask).to(DEV).to(torch.float16)
    got = refine.refine_mask(hg, hm)
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (2, 33, 100)
    assert (_bits(got.cpu().numpy()) == _bits(ref.refine_ref(hg.float().cpu().numpy(), hm.float().cpu().numpy(), 8, 1e-3))).all()
    full = torch.from_numpy(_soft(2, 66, 100)).to(DEV)
    for bad in (dict(radius=2.0), dict(radius=True), dict(radius=-1), dict(radius=65), dict(eps=0.0), dict(eps=2.0),
                dict(eps=float("nan")), dict(grow=257), dict(grow=1.5)):
        with pytest.raises(ValueError):
            refine.refine_mask(gt, full, **bad)
    with pytest.raises(ValueError):
        refine.refine_mask(gt, full[:, :33])
    with pytest.raises(ValueError):
        refine.refine_mask(gt[..., :2], full)
    # radius 0: the grown mask, nothing else
    got = refine.refine_mask(gt, full[:1], radius=0, grow=2).cpu().numpy()
    want = ref.grow_ref(full[0].cpu().numpy(), 2)
    assert got.shape == (2, 66, 100) and (got == want[None]).all()
    # the grow comes first
    got = refine.refine_mask(gt, full, radius=3, eps=1e-3, grow=-1).cpu().numpy()
    grown = np.stack([ref.grow_ref(m, -1) for m in full.cpu().numpy()])
    assert (_bits(got) == _bits(ref.refine_ref(guide, grown, 3, 1e-3))).all()


@functools.lru_cache(maxsize=None)
def _grow_case():
    H, W = 33, 65
    rng = _rng(H, W, 21)
    blobs = np.zeros((H, W), np.float32)
    blobs[5:20, 8:30] = 1.0
    blobs[10:13, 15:18] = 0.0
    blobs[25:31, 40:60] = 0.7
    blobs[2, 63], blobs[30, 2] = 0.5, 0.49999
    masks = np.stack([blobs, (rng.random((H, W)) < 0.03).astype(np.float32), (rng.random((H, W)) < 0.97).astype(np.float32)])
    return masks, {g: np.stack([ref.grow_ref(m, g) for m in masks]) for g in (-5, -1, 1, 5, 40)}


@pytest.mark.parametrize("grow", [-5, -1, 1, 5, 40])
def test_grow_mask_is_the_brute_force_disc(grow):
    masks, want = _grow_case()
    got = refine.grow_mask(torch.from_numpy(masks).to(DEV), grow)
    assert got.dtype == torch.float32 and got.is_cuda and (got.cpu().numpy() == want[grow]).all()
    one = refine.grow_mask(torch.from_numpy(masks[0]).to(DEV), grow)                                               # [H, W]
    assert tuple(one.shape) == (33, 65) and (one.cpu().numpy() == want[grow][0]).all()


def test_grow_mask_keeps_an_empty_and_a_full_mask():
    for level in (0.0, 1.0):
        m = torch.full((2, 33, 65), level, device=DEV)
        for grow in (-40, -1, 1, 40):
            assert torch.equal(refine.grow_mask(m, grow), m), (level, grow)
    soft = torch.from_numpy(_soft(2, 33, 65)).to(DEV)
    assert refine.grow_mask(soft, 0) is soft
    with pytest.raises(ValueError):
        refine.grow_mask(soft, 300)


def test_node_end_to_end_from_host_tensors():
    guide, mask = _guide(2, 48, 40, 3, 9), _blobs(2, 48, 40)
    out, = refine_nodes.LanPaint_MaskRefine().refine(torch.from_numpy(guide), torch.from_numpy(mask), 0, 8, 1e-3)
    assert not out.is_cuda and (_bits(out.numpy()) == _bits(ref.refine_ref(guide, mask, 8, 1e-3))).all()
    out, = refine_nodes.LanPaint_MaskRefine().refine(torch.from_numpy(guide), torch.from_numpy(mask[0]), 3, 2, 1e-2)
    grown = ref.grow_ref(mask[0], 3)[None]
    assert tuple(out.shape) == (2, 48, 40) and (_bits(out.numpy()) == _bits(ref.refine_ref(guide, grown, 2, 1e-2))).all()
