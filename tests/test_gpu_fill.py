"""The masked-area fill and the outpaint canvas on the MI355X (lanpaint_amd.fill, csrc/fill_kernel.hip) against the numpy
restatement tests/fill_ref.py.  The rule fixes every value and the order of every operation, so the device must give the
restatement's values exactly, whatever a launch covers; known pixels and the canvas are compared as bits.  Every comparison covers
every element.  Inputs lie in [0.05, 1): nothing on the way is subnormal."""
import ctypes

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, fill, fill_nodes
from lanpaint_amd._util import raw_stream
from tests import fill_ref
from tests.compare import _raw_bits as _bits
from tests.device import DEV
from tests.image_inputs import _band, _fill_speckle as _speckle, _image, _rng

pytestmark = pytest.mark.gpu
ABOVE = np.nextafter(np.float32(0.5), np.float32(1.0))
# (H, W, C): one pixel, one row, one column; around the 32-pixel tile and two tiles; more than one block each way; a 140 x 150
# hole; thin shapes of 13 and 14 levels (three spans each way) at a few KB.  W % 4 != 0 and C in {1, 2, 5}: the element-wise form.
SHAPES = [(1, 1, 3), (1, 7, 1), (7, 1, 4), (31, 33, 3), (32, 32, 4), (63, 65, 3), (64, 64, 5), (65, 129, 2), (130, 200, 3),
          (160, 200, 3), (1, 2049, 3), (2049, 1, 1), (3, 4100, 4)]


def _hole(Bm, H, W):
    """One hole wider than two tiles along every axis that is long enough for it, or None."""
    r = (10, H - 10) if H >= 85 else (0, H)
    c = (25, W - 25) if W >= 115 else (10, W - 10) if W >= 85 else (0, W)
    if r == (0, H) and c == (0, W):
        return None
    m = np.zeros((Bm, H, W), dtype=np.float32)
    m[:, r[0]:r[1], c[0]:c[1]] = 1.0
    return m


def _corner(Bm, H, W, which):
    m = np.ones((Bm, H, W), dtype=np.float32)
    m[:, (0, 0, H - 1, H - 1)[which], (0, W - 1, 0, W - 1)[which]] = 0.0
    return m


def _edge(Bm, H, W):
    """Exactly 0.5 everywhere -- known -- with a few elements at the next float above it -- masked."""
    rng = _rng(Bm, H, W, 7)
    m = np.full((Bm, H, W), 0.5, dtype=np.float32)
    for p in range(Bm):
        for _ in range(3):
            m[p, rng.integers(H), rng.integers(W)] = ABOVE
    return m


def _nan_mask(Bm, H, W):
    m = _speckle(Bm, H, W, 3)
    m[_rng(Bm, H, W, 4).random((Bm, H, W)) < 0.2] = np.nan          # a NaN is not > 0.5: known
    return m


def _mask_forms(Bm, H, W):
    forms = {"speckle": _speckle(Bm, H, W), "hole": _hole(Bm, H, W), "band": _band(Bm, H, W),
             "all known": np.zeros((Bm, H, W), dtype=np.float32), "all masked": np.ones((Bm, H, W), dtype=np.float32),
             "edge": _edge(Bm, H, W), "nan": _nan_mask(Bm, H, W)}
    for which in range(4):
        forms[f"corner {which}"] = _corner(Bm, H, W, which)
    return {k: v for k, v in forms.items() if v is not None}


def _fill(img, mask):
    return fill.fill_masked(torch.from_numpy(img).to(DEV), torch.from_numpy(mask).to(DEV)).cpu().numpy()


def _check_fill(img, mask, what):
    got = _fill(img, mask)
    want = fill_ref.fill_ref(img, mask)
    assert got.dtype == np.float32 and got.shape == img.shape, what
    bad = got != want
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), float(np.abs(got - want).max()))
    known = np.broadcast_to(~(mask > 0.5), img.shape[:3])
    assert (_bits(got)[known] == _bits(img)[known]).all(), what     # known pixels: the image's bits
    return got


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fill_equals_the_restatement_exactly(shape):
    H, W, C = shape
    for B in (1, 3):
        img = _image(B, H, W, C)
        for name, mask in _mask_forms(B, H, W).items():
            got = _check_fill(img, mask, (shape, B, name))
            if name == "all known" or name == "all masked":
                assert (_bits(got) == _bits(img)).all(), (shape, B, name)
            if name == "speckle":
                assert (_bits(_fill(img, mask)) == _bits(got)).all(), (shape, B, "two calls")
    # batch forms: one mask for three images; a batch whose middle frame alone has no known pixel
    img = _image(3, H, W, C, 5)
    _check_fill(img, _speckle(1, H, W, 9), (shape, "mask_batch 1"))
    mask = _speckle(3, H, W, 11)
    mask[1] = 1.0
    got = _check_fill(img, mask, (shape, "middle frame all masked"))
    assert (_bits(got[1]) == _bits(img[1])).all()


def test_fill_fills_from_the_known_pixels_only():
    """Every filled value lies inside the range of the known values; one known pixel gives a constant image; the image under
    the mask, replaced by NaN, changes nothing."""
    img = _image(2, 130, 200, 3, 2)
    mask = _hole(2, 130, 200)
    got = _fill(img, mask)
    for b in range(2):
        kn = ~(mask[b] > 0.5)
        assert got[b].min() >= img[b][kn].min() and got[b].max() <= img[b][kn].max()
    one = _fill(img, _corner(2, 130, 200, 3))
    assert (one == img[:, -1:, -1:, :]).all()
    for m in (mask, _speckle(2, 130, 200, 13)):
        poisoned = np.where((m > 0.5)[..., None], np.float32(np.nan), img).astype(np.float32)
        assert (_bits(_fill(poisoned, m)) == _bits(_fill(img, m))).all()


@pytest.mark.parametrize("shape", [(160, 200, 3), (3, 4100, 4), (65, 129, 2)], ids=lambda s: "x".join(map(str, s)))
def test_fill_entry_does_not_read_its_workspace_before_writing_it(shape, hip_lib):
    H, W, C = shape
    B = 2
    img, mask = _image(B, H, W, C, 3), _hole(B, H, W)
    mask[1] = _speckle(1, H, W, 17)[0]
    it, mt = torch.from_numpy(img).to(DEV), torch.from_numpy(mask).to(DEV)
    ws_bytes = hip_lib.lp_fill_ws_bytes(B, H, W, C)
    assert ws_bytes == _cabi.fill_ws_bytes(B, H, W, C)
    ws = torch.full((ws_bytes // 4,), float("nan"), dtype=torch.float32, device=DEV)
    out = torch.full_like(it, float("nan"))
    d = _cabi.LpFillDesc(B, H, W, C, B, 0, it.data_ptr(), mt.data_ptr(), out.data_ptr(), ws.data_ptr(), ws_bytes)
    assert hip_lib.lp_mask_fill(ctypes.byref(d), raw_stream(DEV)) == _cabi.LP_OK
    got = out.cpu().numpy()
    assert (_bits(got) == _bits(fill.fill_masked(it, mt).cpu().numpy())).all()
    assert (got == fill_ref.fill_ref(img, mask)).all()


def test_fill_wrapper_takes_views_half_precision_and_a_plain_mask():
    img, mask = _image(2, 66, 100, 3, 4), _speckle(1, 33, 100, 19)
    it = torch.from_numpy(img).to(DEV)
    view = it[:, ::2]                                               # [2, 33, 100, 3], not contiguous
    got = fill.fill_masked(view, torch.from_numpy(mask[0]).to(DEV)).cpu().numpy()       # mask [H, W]
    assert (got == fill_ref.fill_ref(np.ascontiguousarray(img[:, ::2]), mask)).all()
    half = it[:, :33].to(torch.float16)
    got = fill.fill_masked(half, torch.from_numpy(mask).to(DEV))
    assert got.dtype == torch.float32 and got.is_cuda
    assert (got.cpu().numpy() == fill_ref.fill_ref(half.float().cpu().numpy(), mask)).all()


# ---- the outpaint canvas --------------------------------------------------------------------------------------------------------------
def _pad_direct(lib, img, mask, pads, overlap, guard):
    """lp_outpaint_pad into the middle of two buffers of sentinels; returns (canvas, mask) after checking the guards."""
    B, H, W, C = img.shape
    left, top, right, bottom = pads
    Hc, Wc = top + H + bottom, left + W + right
    Bm = 0 if mask is None else mask.shape[0]
    it = torch.from_numpy(img).to(DEV)
    mt = None if mask is None else torch.from_numpy(mask).to(DEV)
    n_img, n_mask = B * Hc * Wc * C, max(Bm, 1) * Hc * Wc
    buf_i = torch.full((n_img + 2 * guard,), -7.0, dtype=torch.float32, device=DEV)
    buf_m = torch.full((n_mask + 2 * guard,), -7.0, dtype=torch.float32, device=DEV)
    d = _cabi.LpOutpaintDesc(B, H, W, C, Bm, left, top, right, bottom, overlap, 0, it.data_ptr(),
                             None if mt is None else mt.data_ptr(), buf_i[guard:].data_ptr(), buf_m[guard:].data_ptr())
    assert lib.lp_outpaint_pad(ctypes.byref(d), raw_stream(DEV)) == _cabi.LP_OK
    bi, bm = buf_i.cpu().numpy(), buf_m.cpu().numpy()
    for b, n in ((bi, n_img), (bm, n_mask)):
        assert (b[:guard] == -7.0).all() and (b[guard + n:] == -7.0).all(), "guard elements overwritten"
    return bi[guard:guard + n_img].reshape(B, Hc, Wc, C), bm[guard:guard + n_mask].reshape(max(Bm, 1), Hc, Wc)


def _pad_masks(B, H, W):
    soft = _rng(B, H, W, 21).random((B, H, W), dtype=np.float32)
    nan = soft.copy()
    nan[_rng(B, H, W, 22).random((B, H, W)) < 0.3] = np.nan
    return {"none": None, "hard 1": _speckle(1, H, W, 23), "soft B": soft, "nan B": nan, "soft 1": soft[:1].copy()}


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("hw", [(12, 16), (13, 14)], ids=lambda s: "x".join(map(str, s)))
def test_outpaint_pad_equals_the_restatement_bit_for_bit(hw, C, hip_lib):
    H, W = hw
    B = 2
    img = _image(B, H, W, C, 6)
    for pads in ((4, 0, 0, 0), (0, 3, 0, 0), (0, 0, 8, 0), (0, 0, 0, 2), (4, 3, 8, 2), (5, 1, 2, 6)):
        for overlap in (0, 5):
            for guard in (64, 3):                                   # 3: outputs off 16-byte alignment, the element-wise form
                for name, mask in _pad_masks(B, H, W).items():
                    canvas, m = _pad_direct(hip_lib, img, mask, pads, overlap, guard)
                    want_c, want_m = fill_ref.pad_ref(img, mask, *pads, overlap)
                    what = (hw, C, pads, overlap, guard, name)
                    assert (_bits(canvas) == _bits(want_c)).all(), what
                    assert (_bits(m) == _bits(want_m)).all(), what


def test_outpaint_pad_wrapper_plans_pads_and_fills():
    img, mask = _image(2, 40, 52, 3, 8), _speckle(2, 40, 52, 25) * np.float32(0.8)
    it, mt = torch.from_numpy(img).to(DEV), torch.from_numpy(mask).to(DEV)
    plan = fill.plan_outpaint(40, 52, 30, 0, 11, 5, 6, 8)
    pads = (plan.left, plan.top, plan.right, plan.bottom)
    assert (plan.height, plan.width) == (48, 96) and pads == (31, 0, 13, 8)
    canvas, m = fill.outpaint_pad(it, mt, 30, 0, 11, 5, overlap=6, multiple_of=8, fill=False)
    want_c, want_m = fill_ref.pad_ref(img, mask, *pads, 6)
    assert canvas.is_cuda and m.is_cuda
    assert (_bits(canvas.cpu().numpy()) == _bits(want_c)).all() and (_bits(m.cpu().numpy()) == _bits(want_m)).all()
    filled, m2 = fill.outpaint_pad(it, mt, 30, 0, 11, 5, overlap=6, multiple_of=8, fill=True)
    assert torch.equal(m2, m)
    assert (_bits(filled.cpu().numpy()) == _bits(fill.fill_masked(canvas, m).cpu().numpy())).all()      # pad, then fill
    assert (filled.cpu().numpy() == fill_ref.fill_ref(want_c, want_m)).all()
    no_mask, m3 = fill.outpaint_pad(it, None, 0, 8, 0, 0, overlap=0, multiple_of=1, fill=False)
    want_c, want_m = fill_ref.pad_ref(img, None, 0, 8, 0, 0, 0)
    assert tuple(m3.shape) == (1, 48, 52)
    assert (_bits(no_mask.cpu().numpy()) == _bits(want_c)).all() and (_bits(m3.cpu().numpy()) == _bits(want_m)).all()


def test_both_nodes_end_to_end_from_host_tensors():
    img, mask = _image(2, 48, 40, 3, 9), _speckle(2, 48, 40, 27)
    it, mt = torch.from_numpy(img), torch.from_numpy(mask)
    out, = fill_nodes.LanPaint_MaskFill().fill(it, mt)
    assert not out.is_cuda and (out.numpy() == fill_ref.fill_ref(img, mask)).all()
    canvas, m = fill_nodes.LanPaint_OutpaintPad().pad(it, left=16, top=0, right=24, bottom=0, overlap=4, multiple_of=8, fill=True,
                                                      mask=mt)
    want_c, want_m = fill_ref.pad_ref(img, mask, 16, 0, 24, 0, 4)
    assert not canvas.is_cuda and not m.is_cuda and tuple(canvas.shape) == (2, 48, 80, 3) and tuple(m.shape) == (2, 48, 80)
    assert (_bits(m.numpy()) == _bits(want_m)).all()
    assert (canvas.numpy() == fill_ref.fill_ref(want_c, want_m)).all()
    inside = canvas.numpy()[:, :, 16:56][~(want_m[:, :, 16:56] > 0.5)]
    assert (_bits(inside) == _bits(img[~(want_m[:, :, 16:56] > 0.5)])).all()       # the original survives outside the band
    canvas, m = fill_nodes.LanPaint_OutpaintPad().pad(it, left=0, top=8, right=0, bottom=0, overlap=0, multiple_of=8, fill=False)
    want_c, want_m = fill_ref.pad_ref(img, None, 0, 8, 0, 0, 0)
    assert (_bits(canvas.numpy()) == _bits(want_c)).all() and (_bits(m.numpy()) == _bits(want_m)).all()
