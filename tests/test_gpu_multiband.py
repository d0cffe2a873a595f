"""The multiband blend on the MI355X (lanpaint_amd.multiband, csrc/multiband_kernel.hip) against the numpy restatement
tests/multiband_ref.py.  The rule fixes every value and the order of every operation, so the device must give the fp32
restatement's values exactly, whatever tile, halo or vector width a launch uses.  Every comparison covers every element.
Inputs lie in [0.05, 1): nothing on the way is subnormal."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, multiband, multiband_nodes
from lanpaint_amd._util import raw_stream
from tests import multiband_ref as ref
from tests.compare import _raw_bits as _bits
from tests.device import DEV
from tests.image_inputs import _band, _image, _multiband_speckle as _speckle, _rng, _soft

pytestmark = pytest.mark.gpu
# (H, W, C): degenerate axes and clamped taps; around one and two tiles (16 for the reduce, 32 for the collapse), odd sizes at
# several levels; W * C % 4 != 0 or C = 5: the element-wise form, the others the float4 form at level 0
SHAPES = [(1, 1, 3), (1, 7, 1), (7, 1, 4), (2, 2, 1), (3, 5, 2), (31, 33, 3), (32, 32, 4), (63, 65, 3), (64, 64, 5), (65, 129, 2),
          (130, 200, 3)]
LEVELS = (0, 1, 2, 5, 12)


def _hole(Bm, H, W):
    """One hole wider than two tiles along every axis that is long enough for it, else over the whole axis."""
    r = (10, H - 10) if H >= 85 else (0, H)
    c = (25, W - 25) if W >= 115 else (10, W - 10) if W >= 85 else (0, W)
    m = np.zeros((Bm, H, W), dtype=np.float32)
    m[:, r[0]:r[1], c[0]:c[1]] = 1.0
    return m


def _corner(Bm, H, W):
    m = np.zeros((Bm, H, W), dtype=np.float32)
    m[:, H - 1, 0] = 1.0
    return m


def _nan_mask(Bm, H, W):
    m = _soft(Bm, H, W, 3)
    m[_rng(Bm, H, W, 4).random((Bm, H, W)) < 0.2] = np.nan
    return m


def _wide(Bm, H, W):
    """Values below 0 and above 1."""
    return (np.float32(3.0) * _soft(Bm, H, W, 5) - np.float32(1.0)).astype(np.float32)


def _mask_forms(Bm, H, W):
    return {"soft": _soft(Bm, H, W), "speckle": _speckle(Bm, H, W), "hole": _hole(Bm, H, W), "band": _band(Bm, H, W),
            "all 0": np.zeros((Bm, H, W), dtype=np.float32), "all 1": np.ones((Bm, H, W), dtype=np.float32),
            "corner": _corner(Bm, H, W), "nan": _nan_mask(Bm, H, W), "wide": _wide(Bm, H, W)}


def _blend(a, b, mask, levels):
    t = [torch.from_numpy(v).to(DEV) for v in (a, b, mask)]
    return multiband.blend_multiband(*t, levels=levels).cpu().numpy()


def _check(a, b, mask, levels, what):
    got = _blend(a, b, mask, levels)
    want = ref.blend_ref(a, b, mask, levels)
    assert got.dtype == np.float32 and got.shape == a.shape, what
    bad = got != want
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), float(np.abs(got - want).max()))
    return got


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_blend_equals_the_restatement_exactly(shape):
    H, W, C = shape
    for B in (1, 3):
        a, b = _image(B, H, W, C, 0), _image(B, H, W, C, 1)
        for name, mask in _mask_forms(B, H, W).items():
            for levels in LEVELS:
                got = _check(a, b, mask, levels, (shape, B, name, levels))
                if name == "all 0":
                    assert (_bits(got) == _bits(a)).all(), (shape, B, levels)
                if name == "soft" and levels == 5:
                    assert (_bits(_blend(a, b, mask, levels)) == _bits(got)).all(), (shape, B, "two calls")
    # one mask for three images
    a, b = _image(3, H, W, C, 5), _image(3, H, W, C, 6)
    for levels in LEVELS:
        _check(a, b, _soft(1, H, W, 9), levels, (shape, "mask_batch 1", levels))


@functools.lru_cache(maxsize=None)
def _reach_case():
    a, b = _image(2, 130, 200, 3, 7), _image(2, 130, 200, 3, 8)
    mask = np.zeros((2, 130, 200), dtype=np.float32)
    mask[0, 64, 100], mask[1, 0, 0], mask[1, 129, 199] = 1.0, 0.5, 2.0
    return a, b, mask


@pytest.mark.parametrize("levels", [0, 1, 2, 3, 4])
def test_the_device_output_reaches_no_further_than_the_bound(levels):
    a, b, mask = _reach_case()
    got = _blend(a, b, mask, levels)
    r = ref.reach(levels)
    yy, xx = np.mgrid[:130, :200]
    far = np.stack([np.maximum(abs(yy - 64), abs(xx - 100)) > r,
                    np.minimum(np.maximum(yy, xx), np.maximum(129 - yy, 199 - xx)) > r])
    assert (_bits(got)[far] == _bits(a)[far]).all() and (got != a).any(axis=(1, 2, 3)).all()
    assert far[0].any() and far[1].any()


def test_equal_images_come_back_as_bits():
    a = _image(3, 65, 129, 3, 9)
    for name, mask in _mask_forms(3, 65, 129).items():
        for levels in (0, 2, 12):
            assert (_bits(_blend(a, a.copy(), mask, levels)) == _bits(a)).all(), (name, levels)


@pytest.mark.parametrize("guard", [64, 3], ids=["aligned", "off 16 bytes"])
@pytest.mark.parametrize("shape", [(130, 200, 3), (64, 64, 4), (65, 129, 2)], ids=lambda s: "x".join(map(str, s)))
def test_entry_does_not_read_its_workspace_before_writing_it_and_stays_inside_out(shape, guard, hip_lib):
    H, W, C = shape
    B, levels = 2, 5
    a, b, mask = _image(B, H, W, C, 3), _image(B, H, W, C, 4), _soft(B, H, W, 17)
    at, bt, mt = (torch.from_numpy(v).to(DEV) for v in (a, b, mask))
    ws_bytes = hip_lib.lp_multiband_ws_bytes(B, H, W, C, levels)
    assert ws_bytes == _cabi.multiband_ws_bytes(B, H, W, C, levels)
    ws = torch.full((ws_bytes // 4,), float("nan"), dtype=torch.float32, device=DEV)
    n = a.size
    buf = torch.full((n + 2 * guard,), float("nan"), dtype=torch.float32, device=DEV)
    out = buf[guard:guard + n]
    assert (out.data_ptr() % 16 == 0) == (guard == 64)
    d = _cabi.LpMultibandDesc(B, H, W, C, B, levels, at.data_ptr(), bt.data_ptr(), mt.data_ptr(), out.data_ptr(), ws.data_ptr(),
                              ws_bytes)
    assert hip_lib.lp_multiband_blend(ctypes.byref(d), raw_stream(DEV)) == _cabi.LP_OK
    host = buf.cpu().numpy()
    assert np.isnan(host[:guard]).all() and np.isnan(host[guard + n:]).all(), "guard elements overwritten"
    got = host[guard:guard + n].reshape(a.shape)
    want = ref.blend_ref(a, b, mask, levels)
    assert not (got != want).any()


def test_wrapper_takes_views_half_precision_and_a_plain_mask():
    a, b, mask = _image(2, 66, 100, 3, 4), _image(2, 66, 100, 3, 5), _soft(1, 33, 100, 19)
    at, bt = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    got = multiband.blend_multiband(at[:, ::2], bt[:, ::2], torch.from_numpy(mask[0]).to(DEV), 3).cpu().numpy()     # mask [H, W]
    assert not (got != ref.blend_ref(np.ascontiguousarray(a[:, ::2]), np.ascontiguousarray(b[:, ::2]), mask, 3)).any()
    ha, hb = at[:, :33].to(torch.float16), bt[:, :33].to(torch.float16)
    got = multiband.blend_multiband(ha, hb, torch.from_numpy(mask).to(DEV))
    assert got.dtype == torch.float32 and got.is_cuda
    assert not (got.cpu().numpy() != ref.blend_ref(ha.float().cpu().numpy(), hb.float().cpu().numpy(), mask, 5)).any()
    for bad in (2.0, True, -1, 17):
        with pytest.raises(ValueError):
            multiband.blend_multiband(at, bt, torch.from_numpy(_soft(2, 66, 100)).to(DEV), bad)
    with pytest.raises(ValueError):
        multiband.blend_multiband(at, bt[:, :33], torch.from_numpy(_soft(2, 66, 100)).to(DEV))
    with pytest.raises(ValueError):
        multiband.blend_multiband(at, bt, torch.from_numpy(mask).to(DEV))


def test_chunks_give_the_bits_of_one_call(monkeypatch):
    a, b, mask = _image(3, 63, 65, 3, 11), _image(3, 63, 65, 3, 12), _soft(3, 63, 65, 13)
    whole = _blend(a, b, mask, 5)
    assert not (whole != ref.blend_ref(a, b, mask, 5)).any()
    per_image = _cabi.multiband_ws_bytes(1, 63, 65, 3, 5)
    for images in (1, 2):
        monkeypatch.setattr(multiband, "WS_CAP_BYTES", images * per_image + 8)
        assert (_bits(_blend(a, b, mask, 5)) == _bits(whole)).all(), images
        assert (_bits(_blend(a, b, mask[:1], 5)) == _bits(_check(a, b, mask[:1], 5, "one mask"))).all(), images
    monkeypatch.setattr(multiband, "WS_CAP_BYTES", 1)               # always at least one image per chunk
    assert (_bits(_blend(a, b, mask, 5)) == _bits(whole)).all()


def test_node_end_to_end_from_host_tensors():
    a, b, mask = _image(2, 48, 40, 3, 9), _image(2, 48, 40, 3, 10), _soft(2, 48, 40, 27)
    out, = multiband_nodes.LanPaint_MultibandBlend().blend(torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(mask), 5)
    assert not out.is_cuda and not (out.numpy() != ref.blend_ref(a, b, mask, 5)).any()
    out, = multiband_nodes.LanPaint_MultibandBlend().blend(torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(mask[0]), 2)
    assert not (out.numpy() != ref.blend_ref(a, b, mask[:1], 2)).any()
