"""The video mask stabilize on the MI355X (lanpaint_amd.stabilize, csrc/stabilize_kernel.hip) against the numpy restatement
tests/stabilize_ref.py.  The rule fixes every value and the order of every floating-point operation, so the device must give the
restatement's bits, whatever instantiation, block or time segment a launch uses: every comparison covers every element and has no
tolerance."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, stabilize, stabilize_nodes, videomask
from lanpaint_amd._util import raw_stream
from tests import stabilize_ref as ref
from tests.compare import _raw_bits as _bits, _same_raw_bits as _same
from tests.device import DEV
from tests.image_checks import _check_q, _device_q
from tests.image_inputs import FORMS, _rng, _stabilize_blobs as _blobs, _stabilize_soft as _soft

pytestmark = pytest.mark.gpu
SEG = _cabi.LP_STAB_SEG_FRAMES                                         # 16: the shortest time segment
MEDIANS, SMOOTHS = (0, 1, 2, 3), (0, 1, 2, 8)                          # the four instantiations: Tm <= 1 or not, Ts <= 2 or not
FEATHERS, GROWS = (0.0, 0.5, 3.0, 64.0), (0.0, 0.5, -0.5, 7.25, -7.25)
# 1, 2, 3 and one under, at and one over 2 Tm + 1 (1..7), 2 Ts + 1 (1..17) and 2 (Tm + Ts) + 1 (1..23) for every pair: 1..24;
# then one under, at and one over one and two time segments, and three segments and a piece
FRAMES = tuple(range(1, 25)) + (2 * SEG - 1, 2 * SEG, 2 * SEG + 1, 3 * SEG + 5)
# (F, H, W): degenerate planes; widths around the 64 lanes of a wave and plane sizes around the 256 pixels of a block; several
# blocks and several segments
SHAPES = [(5, 1, 1), (6, 1, 7), (7, 7, 1), (4, 5, 9), (3, 2, 31), (3, 1, 32), (3, 3, 33), (3, 1, 63), (3, 1, 65), (3, 1, 255),
          (18, 16, 16), (3, 1, 257), (17, 3, 171), (40, 70, 130)]
ONE = np.float32(1.0).view(np.uint32)


def _random_q(F, H, W, seed=5):
    """Signed squared distances as stage 1 could write them: small values of both signs, never 0, values beyond the cap, and
    +-LP_STAB_Q_FAR frames."""
    rng = _rng(F, H, W, seed)
    q = rng.integers(1, 60, (F, H, W)) * rng.choice([-1, 1], (F, H, W))
    far = rng.random((F, H, W)) < 0.1
    q[far] = rng.integers(4000, 2 * 16383 ** 2, int(far.sum())) * rng.choice([-1, 1], int(far.sum()))
    for t in range(F):
        if rng.random() < 0.15:
            q[t] = rng.choice([-1, 1]) * _cabi.LP_STAB_Q_FAR
    return q.astype(np.int32)


@pytest.mark.parametrize("smooth", SMOOTHS)
def test_every_frame_count_and_radius_pair_equals_the_restatement(smooth):
    H, W = 5, 9
    for F in FRAMES:
        q = _random_q(F, H, W)
        grow, feather = GROWS[F % len(GROWS)], FEATHERS[F % len(FEATHERS)]
        _check_q(torch.from_numpy(q).to(DEV), q, [(tm, smooth, grow, feather) for tm in MEDIANS], ("frames", F))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stabilize_equals_the_restatement_bit_for_bit(shape):
    F, H, W = shape
    for name in ("soft", "blobs"):
        mask = FORMS[name](F, H, W)
        q_ref = ref.signed_d2(mask)
        q_dev = _device_q(mask)
        assert q_dev.dtype == torch.int32 and (q_dev.cpu().numpy() == q_ref).all(), (shape, name, "stage 1")
        got = _check_q(q_dev, q_ref, [(0, 0, 0.0, 0.0), (1, 2, 0.0, 0.0), (2, 1, 0.5, 3.0), (3, 8, -0.5, 0.5), (1, 8, 0.0, 0.0),
                                      (3, 2, 7.25, 64.0)], (shape, name))
        _same(got[0], (mask >= np.float32(0.5)).astype(np.float32), (shape, name, "radii 0: the binarised input"))
        whole = stabilize.stabilize_masks(torch.from_numpy(mask).to(DEV)).cpu().numpy()
        _same(whole, got[1], (shape, name, "stabilize_masks"))
        _same(stabilize.stabilize_masks(torch.from_numpy(mask).to(DEV)).cpu().numpy(), whole, (shape, name, "two calls"))


@pytest.mark.parametrize("form", list(FORMS))
def test_every_mask_form_equals_the_restatement(form):
    F, H, W = 20, 33, 65
    mask = FORMS[form](F, H, W)
    q_ref = ref.signed_d2(mask)
    q_dev = _device_q(mask)
    assert (q_dev.cpu().numpy() == q_ref).all(), (form, "stage 1")
    cases = [(tm, ts, 0.0, 0.0) for tm, ts in ((0, 0), (1, 2), (2, 8), (3, 1))] + [(1, 2, 0.0, 3.0), (3, 8, 0.0, 64.0)]
    got = _check_q(q_dev, q_ref, cases, form)
    if form == "all 0":
        assert (_bits(got) == 0).all()
    if form == "all 1":
        assert (_bits(got) == ONE).all()
    if form == "single":                                             # one frame long: gone with any median
        assert got[0].sum() == 1 and (_bits(got[1:4]) == 0).all()


@functools.lru_cache(maxsize=None)
def _grow_case():
    mask = _blobs(19, 33, 65, 7)
    return mask, ref.signed_d2(mask)


@pytest.mark.parametrize("feather", FEATHERS)
def test_every_grow_and_feather_equals_the_restatement(feather):
    mask, q_ref = _grow_case()
    q_dev = _device_q(mask)
    got = _check_q(q_dev, q_ref, [(tm, ts, grow, feather) for grow in GROWS for tm, ts in ((1, 2), (3, 8))], ("feather", feather))
    assert (got >= 0).all() and (got <= 1).all()
    if feather == 0.0:
        assert np.isin(got, (0.0, 1.0)).all() and (got[6] >= got[0]).all() and (got[8] <= got[0]).all()   # grow 7.25, -7.25


def test_equal_frames_give_the_binarised_frame_for_every_radius_pair():
    F, H, W = 21, 12, 37
    frame = _soft(1, H, W, 9)
    mask = np.repeat(frame, F, axis=0)
    q_dev = _device_q(mask)
    want = np.repeat((frame >= np.float32(0.5)).astype(np.float32), F, axis=0)
    got = torch.stack([stabilize.stabilize_q(q_dev, tm, ts) for tm in MEDIANS for ts in SMOOTHS]).cpu().numpy()
    for g in got:
        _same(g, want, "equal frames")


def test_signed_d2_alone_equals_the_restatement(hip_lib):
    F, H, W = 6, 9, 21
    rng = _rng(F, H, W, 11)
    planes = rng.integers(1, 900, (F, 2, H, W)).astype(np.int32)
    fg = rng.random((F, H, W)) < 0.5
    planes[:, 0][fg] = 0                                              # a pixel is at distance 0 from its own kind
    planes[:, 1][~fg] = 0
    planes[1, 0], planes[1, 1] = _cabi.LP_VMASK_D2_NONE, 0           # an empty frame
    planes[4, 0], planes[4, 1] = 0, _cabi.LP_VMASK_D2_NONE           # a full frame
    planes[5, 0, 3, 4], planes[5, 1, 3, 4] = 2 * 16383 ** 2, 0       # the largest squared distance there is
    d2 = torch.from_numpy(planes).to(DEV)
    guard = 5
    buf = torch.full((F * H * W + 2 * guard,), 77, dtype=torch.int32, device=DEV)
    q = buf[guard:guard + F * H * W]
    assert hip_lib.lp_mask_signed_d2(d2.data_ptr(), F, H, W, q.data_ptr(), raw_stream(DEV)) == _cabi.LP_OK
    host = buf.cpu().numpy()
    assert (host[:guard] == 77).all() and (host[-guard:] == 77).all(), "guard elements overwritten"
    want = ref.signed_from_planes(planes)
    assert (host[guard:-guard].reshape(F, H, W) == want).all()
    assert (want[1] == -_cabi.LP_STAB_Q_FAR).all() and (want[4] == _cabi.LP_STAB_Q_FAR).all()
    # and on the planes the EDT writes
    mask = np.concatenate([_blobs(4, 9, 21), np.zeros((1, 9, 21), np.float32), np.ones((1, 9, 21), np.float32)])
    d2, _, _ = videomask.keyframe_edt(torch.from_numpy(mask).to(DEV))
    q = torch.empty((6, 9, 21), dtype=torch.int32, device=DEV)
    assert hip_lib.lp_mask_signed_d2(d2.data_ptr(), 6, 9, 21, q.data_ptr(), raw_stream(DEV)) == _cabi.LP_OK
    assert (q.cpu().numpy() == ref.signed_from_planes(d2.cpu().numpy())).all() and (q.cpu().numpy() == ref.signed_d2(mask)).all()


@pytest.mark.parametrize("guard", [64, 3], ids=["aligned", "off 16 bytes"])
@pytest.mark.parametrize("shape", [(35, 7, 37), (3, 1, 257)], ids=lambda s: "x".join(map(str, s)))
def test_entry_stays_inside_out(shape, guard, hip_lib):
    F, H, W = shape
    q = _random_q(F, H, W, 13)
    qt = torch.from_numpy(q).to(DEV)
    n = F * H * W
    buf = torch.full((n + 2 * guard,), float("nan"), dtype=torch.float32, device=DEV)
    out = buf[guard:guard + n]
    d = _cabi.LpStabilizeDesc(F, H, W, 3, 8, 0, 0.5, 3.0, qt.data_ptr(), out.data_ptr())
    assert hip_lib.lp_mask_stabilize(ctypes.byref(d), raw_stream(DEV)) == _cabi.LP_OK
    host = buf.cpu().numpy()
    assert np.isnan(host[:guard]).all() and np.isnan(host[guard + n:]).all(), "guard elements overwritten"
    _same(host[guard:guard + n].reshape(F, H, W), ref.stabilize_q_ref(q, 3, 8, 0.5, 3.0), shape)


def test_chunks_give_the_bits_of_one_call(monkeypatch):
    mask = _blobs(7, 21, 40, 15)
    t = torch.from_numpy(mask).to(DEV)
    whole = stabilize.stabilize_masks(t, 1, 2, 0.5, 3.0).cpu().numpy()
    _same(whole, ref.stabilize_ref(mask, 1, 2, 0.5, 3.0), "one chunk")
    per_frame = videomask.EDT_BYTES_PER_PIXEL * 21 * 40
    for frames in (1, 2, 3):
        monkeypatch.setattr(stabilize, "WS_CAP_BYTES", frames * per_frame + 8)
        _same(stabilize.stabilize_masks(t, 1, 2, 0.5, 3.0).cpu().numpy(), whole, frames)
    monkeypatch.setattr(stabilize, "WS_CAP_BYTES", 1)                 # always at least one frame per chunk
    _same(stabilize.stabilize_masks(t, 1, 2, 0.5, 3.0).cpu().numpy(), whole, "cap 1")


def test_wrapper_takes_views_half_precision_and_one_frame():
    mask = _soft(6, 40, 31, 17)
    t = torch.from_numpy(mask).to(DEV)
    _same(stabilize.stabilize_masks(t[:, ::2]).cpu().numpy(), ref.stabilize_ref(np.ascontiguousarray(mask[:, ::2])), "a view")
    half = t.to(torch.float16)
    got = stabilize.stabilize_masks(half, 2, 3)
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (6, 40, 31)
    _same(got.cpu().numpy(), ref.stabilize_ref(half.float().cpu().numpy(), 2, 3), "fp16")
    one = stabilize.stabilize_masks(t[0], 3, 8)                       # [H, W]: one frame
    assert tuple(one.shape) == (1, 40, 31)
    _same(one.cpu().numpy(), (mask[:1] >= np.float32(0.5)).astype(np.float32), "one frame")
    for bad in (t[0, 0], t[None], t[:0], t[:, :0]):
        with pytest.raises(ValueError):
            stabilize.stabilize_masks(bad)
    with pytest.raises(ValueError):
        stabilize.stabilize_q(t)                                      # not int32


def test_node_returns_what_the_module_returns_on_the_inputs_device():
    mask = _blobs(9, 24, 40, 19)
    node = stabilize_nodes.LanPaint_VideoMaskStabilize()
    want = ref.stabilize_ref(mask, 1, 2, 0.5, 3.0)
    out, = node.stabilize(torch.from_numpy(mask), 1, 2, 0.5, 3.0)
    assert not out.is_cuda and out.dtype == torch.float32
    _same(out.numpy(), want, "host in, host out")
    on = torch.from_numpy(mask).to(DEV)
    out, = node.stabilize(on, 1, 2, 0.5, 3.0)
    assert out.device == on.device and torch.equal(out, stabilize.stabilize_masks(on, 1, 2, 0.5, 3.0))
    _same(out.cpu().numpy(), want, "device in, device out")
    out, = node.stabilize(torch.from_numpy(mask))                     # the defaults: median 1, smooth 2
    _same(out.numpy(), ref.stabilize_ref(mask), "defaults")
