"""lanpaint_amd._hostcall, the plumbing the image-space modules share, as far as it runs without a device: the argument checks,
the mask and image shape rules and the chunk arithmetic."""
import pytest
import torch

from lanpaint_amd import _cabi, _hostcall as hc

CPU = torch.device("cpu")


def test_int_in_takes_both_ends_and_nothing_else():
    assert hc.int_in(-3, -3, 7, "v") == -3 and hc.int_in(7, -3, 7, "v") == 7 and hc.int_in(0, 0, 0, "v") == 0
    for bad in (-4, 8, True, False, 1.0, float("nan"), "1", None):
        with pytest.raises(ValueError, match=r"grow must be an integer in -3\.\.7"):
            hc.int_in(bad, -3, 7, "grow")


def test_float_in_takes_both_ends_and_integers_and_nothing_else():
    assert hc.float_in(-0.5, -0.5, 2, "v") == -0.5 and hc.float_in(2, -0.5, 2, "v") == 2.0
    assert isinstance(hc.float_in(1, 0, 2, "v"), float)
    for bad in (-0.75, 2.25, True, float("nan"), float("inf"), "1.0", None):
        with pytest.raises(ValueError, match=r"feather must be a number in -0\.5\.\.2"):
            hc.float_in(bad, -0.5, 2, "feather")


def test_mask3_lifts_a_plane_and_refuses_four_axes():
    assert tuple(hc.mask3(torch.zeros(4, 5)).shape) == (1, 4, 5)
    m = torch.zeros(3, 4, 5)
    assert hc.mask3(m) is m
    with pytest.raises(ValueError, match="mask must be"):
        hc.mask3(torch.zeros(1, 3, 4, 5))


def test_image4_with_and_without_a_batch_limit():
    t = torch.zeros(2, 3, 4, 3)
    assert hc.image4(t, "image") is t and hc.image4(t, "image", 2) is t
    with pytest.raises(ValueError, match=r"batch 1\.\.1"):
        hc.image4(t, "image", 1)
    many = torch.zeros(1, 1, 1, 1).expand(hc.MAX_BATCH + 1, 1, 1, 1)
    assert hc.image4(many, "image") is many                          # no limit: the caller chunks
    with pytest.raises(ValueError, match=r"detail .*batch 1\.\.65535"):
        hc.image4(many, "detail", hc.MAX_BATCH)
    wide = torch.zeros(1, 1, 1, 1).expand(1, 1, _cabi.LP_DETAIL_MAX_SIDE + 1, 1)
    for bad in (torch.zeros(3, 4, 3), torch.zeros(0, 3, 4, 3), torch.zeros(1, 3, 0, 3), wide,
                torch.zeros(1, 2, 2, _cabi.LP_DETAIL_MAX_CHANNELS + 1)):
        with pytest.raises(ValueError, match="image"):
            hc.image4(bad, "image")


def test_mask_for_takes_one_plane_or_one_per_image():
    for planes in ((4, 5), (1, 4, 5), (3, 4, 5)):
        m = hc.mask_for(torch.ones(planes, dtype=torch.float16), 3, 4, 5, CPU)
        assert m.dtype == torch.float32 and m.is_contiguous() and tuple(m.shape) == ((1, 4, 5) if len(planes) == 2 else planes)
    view = torch.rand(3, 4, 10)[:, :, ::2]
    m = hc.mask_for(view, 3, 4, 5, CPU)
    assert m.is_contiguous() and torch.equal(m, view)
    for bad in ((2, 4, 5), (3, 5, 4), (3, 4, 6), (4, 4, 5)):
        with pytest.raises(ValueError, match="mask shape"):
            hc.mask_for(torch.zeros(bad), 3, 4, 5, CPU)


def test_chunks():
    assert list(hc.chunks(7, 10, 1000)) == [(0, 7)]                                          # the whole batch
    assert list(hc.chunks(6, 10, 20)) == [(0, 2), (2, 2), (4, 2)]                            # an exact multiple
    assert list(hc.chunks(7, 10, 38)) == [(0, 3), (3, 3), (6, 1)]                            # a remainder
    assert list(hc.chunks(3, 10, 1)) == [(0, 1), (1, 1), (2, 1)]                             # a cap below one item
    assert list(hc.chunks(65536, 1, 1 << 60)) == [(0, 65535), (65535, 1)]                    # a launch's batch limit
    assert list(hc.chunks(0, 10, 1000)) == []
    for n, per, cap in ((7, 10, 38), (65536, 1, 1 << 60), (5, 3, 1)):
        first = list(hc.chunks(n, per, cap))[0][1]
        assert first == min(n, 65535, max(1, cap // per))
        assert all(c <= first for _, c in hc.chunks(n, per, cap))                            # a workspace for the first serves all


def test_no_device_means_an_error_not_a_fallback(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    t = torch.zeros(2, 2)
    with pytest.raises(RuntimeError, match=r"lanpaint_amd\.refine runs on a HIP device only; no CPU fallback \(mask is not"):
        hc.require_hip(t, "mask", "lanpaint_amd.refine")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hc.require_hip([[0.0]], "mask", "lanpaint_amd.refine")
    with pytest.raises(RuntimeError, match="no CPU fallback") as e:
        hc.node_device(t)
    assert "Detailer" not in str(e.value)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hc.node_device(t, "cpu")
    assert hc.node_device(t, "cuda:1") == torch.device("cuda", 1)      # a named HIP device is taken at its word


def test_node_mask_lifts_a_plane():
    assert tuple(hc.node_mask(torch.zeros(4, 5), CPU).shape) == (1, 4, 5)
    assert tuple(hc.node_mask(torch.zeros(2, 4, 5), CPU).shape) == (2, 4, 5)
