"""The grain match, the parts that need no device: the restatement (tests/grain_ref.py) checked on its own -- Philox against
Random123's vector, the kernel table by convolution, the white value's variance, and the case the rule was tried on --, the four C
entries' argument checks (made before any HIP call), the node's protocol and the no-fallback errors.  Layouts, constants and names
against the header are tests/test_cabi_mirror.py's, for the whole C ABI."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, grain, grain_nodes
from tests import grain_ref as ref
from tests.compare import _f32_bits as _bits

NEW_ENTRIES = ("lp_grain_stats", "lp_grain_fit", "lp_grain_field", "lp_grain_apply")


# ---- the restatement on its own -------------------------------------------------------------------------------------------------------
def test_philox_known_answer():
    words = ref.philox4x32_10(0, 0, 0)
    assert [int(w) for w in words] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    # Random123's other two vectors: all ones, and the digits of pi
    ones = (1 << 64) - 1
    assert [int(w) for w in ref.philox4x32_10(ones, ones, ones)] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    pi = ref.philox4x32_10(0x85a308d3243f6a88, 0x0370734413198a2e, 0x299f31d0a4093822)
    assert [int(w) for w in pi] == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    many = ref.philox4x32_10(np.arange(5), 3, 7)                       # arrays broadcast, one block per counter
    assert [int(w[4]) for w in many] == [int(w) for w in ref.philox4x32_10(4, 3, 7)]


def test_the_kernel_table_is_what_convolution_gives():
    assert ref.N5.shape == (5, 5) and (ref.N5[::2, ::2] == ref.N3).all() and ref.N5.sum() == 0 and np.abs(ref.N5).sum() == 16
    yy, xx = np.mgrid[:5, :5]
    for plane in (np.ones((5, 5)), yy, xx, 3 * yy - 2 * xx + 7):       # blind to planes
        assert (ref.N5 * plane).sum() == 0 and (ref.N3 * plane[1:4, 1:4]).sum() == 0
    for s, k in enumerate(ref.KERNELS):
        assert (k ** 2).sum() == ref.SUM_K2[s]
        assert (ref.full_conv(ref.N3, k) ** 2).sum() == ref.S1[s]
        assert (ref.full_conv(ref.N5, k) ** 2).sum() == ref.S2[s]
    assert ref.SUM_K2 == (1, 36, 4900) and ref.S1 == (36, 36, 784) and ref.S2 == (36, 784, 39204)
    # the size thresholds are the geometric means of S2 / S1 of neighbouring sizes
    r = [ref.S2[s] / ref.S1[s] for s in range(3)]
    assert abs(np.sqrt(r[0] * r[1]) - 14 / 3) < 1e-12 and abs(np.sqrt(r[1] * r[2]) - 33) < 1e-12


def test_the_white_value_has_the_variance_the_fit_assumes():
    w = ref.white(3, 252, 252, 1, seed=11)                             # 256 * 256 = 65536 draws
    assert w.size == 65536 and w.min() >= -510 and w.max() <= 510
    var = float((w.astype(np.float64) ** 2).mean())
    print("white variance", var, "mean", w.mean())
    assert abs(var - ref.WHITE_VAR) <= 0.02 * ref.WHITE_VAR and abs(w.mean()) < 3.0
    assert ref.WHITE_VAR == 4 * (256 ** 2 - 1) // 12


def test_the_field_depends_on_its_coordinates_only():
    g = ref.grain_field(3, 6, 7, 5, 2, seed=9, frame0=4)
    assert g.dtype == np.int32 and g.shape == (3, 6, 7, 5)
    assert (ref.grain_field(1, 6, 7, 5, 2, seed=9, frame0=5)[0] == g[1]).all()
    mono = ref.grain_field(2, 6, 7, 5, 1, seed=9, monochrome=True)
    assert (mono == mono[..., :1]).all() and (mono[..., 0] == ref.grain_field(2, 6, 7, 1, 1, seed=9)[..., 0]).all()
    w = ref.white(0, 6, 7, 5, 9)
    assert (ref.grain_field(1, 6, 7, 5, 0, seed=9)[0] == w[2:-2, 2:-2]).all()
    assert (ref.grain_field(1, 6, 7, 5, 0, seed=10) != g[:1]).any()


def test_stats_by_hand_on_a_small_image():
    img = np.zeros((1, 5, 5, 1), np.float32)
    img[0, 2, 2, 0] = 10 / 255
    s = ref.grain_stats(img, flat=255)
    assert s.shape == (1, 1, 8, 3) and s[0, 0, 0].tolist() == [1, 40 * 40, 40 * 40] and not s[0, 0, 1:].any()
    assert not ref.grain_stats(img, flat=9).any() and ref.grain_stats(img, flat=10)[0, 0, 0, 0] == 1
    assert not ref.grain_stats(img[:, :4], flat=255).any()             # a side under 5
    mask = np.ones((1, 5, 5), np.float32)
    assert ref.grain_stats(img, mask, ref.INSIDE, 255)[0, 0, 0, 0] == 1
    assert not ref.grain_stats(img, mask, ref.OUTSIDE, 255, 0).any()
    mask[0, 0, 0] = 0.5                                                # not > 0.5: the window is no longer inside
    assert not ref.grain_stats(img, mask, ref.INSIDE, 255).any()
    far = np.zeros((1, 5, 5), np.float32)
    far[0, 0, 0] = 1.0
    assert ref.grain_stats(img, far, ref.OUTSIDE, 255, 1)[0, 0, 0, 0] == 1 and not ref.grain_stats(img, far, ref.OUTSIDE, 255, 2).any()
    bright = np.full((1, 5, 5, 1), 1.0, np.float32)
    assert ref.grain_stats(bright, flat=0)[0, 0, 7].tolist() == [1, 0, 0]


def _binomial_noise(rng, shape, size, sigma):
    """Gaussian noise of standard deviation sigma, white or filtered with k_size (and scaled back to sigma)."""
    H, W, C = shape
    n = rng.normal(0.0, 1.0, (H + 4, W + 4, C))
    k = ref.KERNELS[size].astype(np.float64)
    out = np.zeros(shape)
    for dy in range(-size, size + 1):
        for dx in range(-size, size + 1):
            out += k[dy + size, dx + size] * n[2 + dy:2 + dy + H, 2 + dx:2 + dx + W]
    return sigma * out / np.sqrt(ref.SUM_K2[size])


@functools.lru_cache(maxsize=None)
def _trial(size):
    """The case the rule was tried on: a 128 x 128 x 3 ramp 0.2..0.8 with noise of 0.03, removed under an 80 x 80 mask."""
    rng = np.random.default_rng(100 + size)
    H = W = 128
    ramp = np.broadcast_to(np.linspace(0.2, 0.8, W)[None, :, None], (H, W, 3))
    noise = _binomial_noise(rng, (H, W, 3), size, 0.03)
    mask = np.zeros((1, H, W), np.float32)
    mask[0, 24:104, 24:104] = 1.0
    image = (ramp + noise * (1.0 - mask[0][..., None])).astype(np.float32)[None]
    return image, mask, noise


@pytest.mark.parametrize("size", [0, 1, 2])
def test_the_restatement_does_its_job(size):
    image, mask, noise = _trial(size)
    gen = ref.grain_stats(image, mask, ref.INSIDE, 255)
    outside = ref.grain_stats(image, mask, ref.OUTSIDE, 255, 8)
    amp, sizes = ref.grain_fit(gen, outside)
    assert sizes.tolist() == [size]
    out = ref.match(image, mask, flat=255, seed=5)
    assert out.dtype == np.float32 and out.shape == image.shape
    keep = mask[0] == 0
    assert (_bits(out)[0][keep] == _bits(image)[0][keep]).all()
    inner = np.zeros((128, 128), bool)
    inner[26:102, 26:102] = True                                      # the mask eroded by 2
    added = (out[0].astype(np.float64) - image[0].astype(np.float64))[inner] * 255.0
    true = noise[inner] * 255.0
    print("size", size, "added std", added.std(), "true std", true.std())
    assert abs(added.std() - true.std()) <= 0.10 * true.std()
    assert (_bits(ref.match(image, mask, flat=255, seed=5)) == _bits(out)).all()
    assert (_bits(ref.match(image, mask, flat=255, seed=5, strength=0.0)) == _bits(image)).all()


def test_fit_branches_by_hand():
    K = ref.K
    def table(rows):                                                   # {(c, k): (n, s1, s2)} -> [1, C, K, 3]
        C = 1 + max(c for c, _ in rows)
        t = np.zeros((1, C, K, 3), np.int64)
        for (c, k), v in rows.items():
            t[0, c, k] = v
        return t
    none = table({(0, 0): (63, 10 ** 6, 10 ** 6)})
    some = table({(0, 3): (64, 64 * 360, 64 * 360)})
    amp, size = ref.grain_fit(none, none)
    assert not amp.any() and size.tolist() == [0]                      # no valid reference band: amplitude 0
    amp, size = ref.grain_fit(none, some)                              # no valid generated band: Egen = 0; one band serves all
    want = np.float32(np.sqrt(720.0 / (ref.WHITE_VAR * 72)) / 255.0)
    assert size.tolist() == [0] and (amp == want).all() and amp.dtype == np.float32
    amp, size = ref.grain_fit(some, some)                              # nothing is missing: A <= 0
    assert not amp.any() and size.tolist() == [0]
    two = table({(0, 1): (100, 100 * 36, 100 * 36), (0, 6): (100, 100 * 3600, 100 * 3600)})
    amp, _ = ref.grain_fit(none, two, size=0)
    assert (amp[0, 0, :4] == amp[0, 0, 1]).all() and (amp[0, 0, 4:] == amp[0, 0, 6]).all() and amp[0, 0, 3] < amp[0, 0, 4]
    for s, (s1, s2) in enumerate(zip(ref.S1, ref.S2)):                 # a grain of size s and unit amplitude is recognised
        t = table({(0, 2): (1000, 1000 * ref.WHITE_VAR * s1, 1000 * ref.WHITE_VAR * s2)})
        amp, size = ref.grain_fit(none, t)
        assert size.tolist() == [s] and amp[0, 0, 0] == np.float32(min(1.0, 64 / np.sqrt(ref.WHITE_VAR * ref.SUM_K2[s])) / 255.0)
    amp, _ = ref.grain_fit(none, some, strength=2.0, size=2)
    assert (amp == np.float32(2.0 * np.sqrt(720.0 / (ref.WHITE_VAR * 39988)) / 255.0)).all()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_grain_entries_reject_bad_arguments_without_a_device(hip_lib):
    C, E, U = ctypes, _cabi.LP_E_INVALID, _cabi.LP_E_UNSUPPORTED
    p, q, r, s, t = (C.c_void_p(256 * k) for k in range(1, 6))         # never dereferenced: validation comes before any HIP call
    side, chan = _cabi.LP_DETAIL_MAX_SIDE, _cabi.LP_DETAIL_MAX_CHANNELS
    shape_changes = ({"batch": 0}, {"batch": -1}, {"height": 0}, {"height": side + 1}, {"width": 0}, {"width": side + 1},
                     {"channels": 0}, {"channels": chan + 1})
    for name in NEW_ENTRIES:
        assert getattr(hip_lib, name)(None, None) == E, name

    good = dict(batch=2, height=40, width=50, channels=3, mask_batch=1, margin=8, flat=64, region=_cabi.LP_GRAIN_REGION_OUTSIDE,
                image=p, mask=q, stats=r)
    for change in shape_changes + ({"margin": -1}, {"margin": 26}, {"flat": -1}, {"flat": 256}, {"region": -1}, {"region": 3},
                                   {"image": None}, {"stats": None}, {"mask": None}, {"mask_batch": 0}, {"mask_batch": 3},
                                   {"mask": None, "region": _cabi.LP_GRAIN_REGION_INSIDE}):
        assert hip_lib.lp_grain_stats(C.byref(_cabi.LpGrainStatsDesc(**{**good, **change})), None) == E, change
    assert hip_lib.lp_grain_stats(C.byref(_cabi.LpGrainStatsDesc(**{**good, "batch": 65536, "mask_batch": 65536})), None) == U

    good = dict(batch=6, ref_batch=6, channels=3, clip_frames=3, size=-1, strength=1.0, gen=p, ref=q, amp=r, size_out=s)
    nan, inf = float("nan"), float("inf")
    for change in ({"batch": 0}, {"batch": -1}, {"ref_batch": 0}, {"channels": 0}, {"channels": chan + 1}, {"clip_frames": -1},
                   {"clip_frames": 4}, {"clip_frames": 7}, {"size": -2}, {"size": 3}, {"strength": -0.1}, {"strength": 2.5},
                   {"strength": nan}, {"strength": inf}, {"gen": None}, {"ref": None}, {"amp": None}, {"size_out": None}):
        assert hip_lib.lp_grain_fit(C.byref(_cabi.LpGrainFitDesc(**{**good, **change})), None) == E, change
    assert hip_lib.lp_grain_fit(C.byref(_cabi.LpGrainFitDesc(**{**good, "batch": 65536, "clip_frames": 0})), None) == U
    assert hip_lib.lp_grain_fit(C.byref(_cabi.LpGrainFitDesc(**{**good, "ref_batch": 65536})), None) == U

    good = dict(batch=2, height=40, width=50, channels=3, size=1, monochrome=0, frame0=0, seed=1, out=p)
    for change in shape_changes + ({"size": -1}, {"size": 3}, {"frame0": -1}, {"frame0": _cabi.LP_GRAIN_MAX_FRAME0 + 1},
                                   {"out": None}):
        assert hip_lib.lp_grain_field(C.byref(_cabi.LpGrainFieldDesc(**{**good, **change})), None) == E, change
    assert hip_lib.lp_grain_field(C.byref(_cabi.LpGrainFieldDesc(**{**good, "batch": 65536})), None) == U

    good = dict(batch=2, height=40, width=50, channels=3, mask_batch=2, monochrome=0, frame0=0, seed=1, image=p, mask=q, amp=r,
                size=s, out=t)
    for change in shape_changes + ({"mask_batch": 0}, {"mask_batch": 3}, {"frame0": -1},
                                   {"frame0": _cabi.LP_GRAIN_MAX_FRAME0 + 1}, {"image": None}, {"mask": None}, {"amp": None},
                                   {"size": None}, {"out": None}, {"out": p}):
        assert hip_lib.lp_grain_apply(C.byref(_cabi.LpGrainApplyDesc(**{**good, **change})), None) == E, change
    assert hip_lib.lp_grain_apply(C.byref(_cabi.LpGrainApplyDesc(**{**good, "batch": 65536, "mask_batch": 1})), None) == U


def test_the_grain_kernels_are_a_source_of_the_build():
    from lanpaint_amd import build
    assert "grain_kernel.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "grain_kernel.hip"))


# ---- the wrapper and the node ---------------------------------------------------------------------------------------------------------
def test_grain_refuses_cpu_tensors_and_bad_arguments():
    image, mask = torch.zeros(2, 16, 16, 3), torch.zeros(2, 16, 16)
    table = torch.zeros(2, 3, 8, 3, dtype=torch.int64)
    for call in (lambda: grain.match(image, mask), lambda: grain.grain_stats(image), lambda: grain.grain_fit(table, table),
                 lambda: grain.grain_apply(image, mask, torch.zeros(2, 3, 8), torch.zeros(2, dtype=torch.int32)),
                 lambda: grain.match(image.numpy(), mask)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    # the numbers are checked before a tensor is looked at
    for bad in (dict(strength=-0.1), dict(strength=2.5), dict(strength=float("nan")), dict(strength="1"), dict(size="huge"),
                dict(size=3), dict(size=-2), dict(size=1.0), dict(flat=-1), dict(flat=256), dict(flat=1.5), dict(margin=-1),
                dict(margin=26), dict(seed=-1), dict(seed=1 << 64), dict(seed=0.5), dict(frame0=-1), dict(frame0=(1 << 30) + 1),
                dict(clip_frames=-1)):
        with pytest.raises(ValueError):
            grain.match(image, mask, **bad)
    for bad in (dict(region="near"), dict(flat=256), dict(margin=26)):
        with pytest.raises(ValueError):
            grain.grain_stats(image, mask, **bad)
    for bad in (dict(size=0, seed=-1), dict(size=3), dict(size=-1), dict(size=0, frame0=-1)):
        with pytest.raises(ValueError):
            grain.grain_field((1, 8, 8, 3), **bad)
    for shape in ((0, 8, 8, 3), (1, 8, 8, 65), (1, 0, 8, 3)):
        with pytest.raises(ValueError):
            grain.grain_field(shape, 0)
    for inside in (dict(strength=0), dict(strength=2.0, size="coarse"), dict(size=-1, flat=0, margin=25, seed=(1 << 64) - 1)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            grain.match(image, mask, **inside)
    assert grain.SIZES == {"auto": -1, "fine": 0, "medium": 1, "coarse": 2}


def test_grain_node_protocol_and_own_mappings():
    node = grain_nodes.LanPaint_GrainMatch
    assert grain_nodes.NODE_CLASS_MAPPINGS == {"LanPaint_GrainMatch": node}
    assert grain_nodes.NODE_DISPLAY_NAME_MAPPINGS == {"LanPaint_GrainMatch": "LanPaint Grain Match"}
    types = node.INPUT_TYPES()
    req, opt = types["required"], types["optional"]
    assert list(types) == ["required", "optional"] and list(opt) == ["reference"] and opt["reference"][0] == "IMAGE"
    assert list(req) == ["image", "mask", "strength", "grain_size", "monochrome", "flat", "margin", "seed", "clip_frames"]
    assert req["image"][0] == "IMAGE" and req["mask"][0] == "MASK"
    assert req["strength"][0] == "FLOAT" and req["strength"][1] == {**req["strength"][1], "default": 1.0, "min": 0.0, "max": 2.0}
    assert req["grain_size"][0] == ["auto", "fine", "medium", "coarse"] and req["grain_size"][1]["default"] == "auto"
    assert set(req["grain_size"][0]) == set(grain.SIZES)
    assert req["monochrome"][0] == "BOOLEAN" and req["monochrome"][1]["default"] is False
    assert req["flat"][0] == "INT" and req["flat"][1] == {**req["flat"][1], "default": 64, "min": 0, "max": 255}
    assert req["margin"][0] == "INT" and req["margin"][1] == {**req["margin"][1], "default": 8, "min": 0, "max": 25}
    assert req["seed"][0] == "INT" and req["seed"][1] == {**req["seed"][1], "default": 0, "min": 0, "max": (1 << 64) - 1}
    assert req["clip_frames"][0] == "INT" and req["clip_frames"][1] == {**req["clip_frames"][1], "default": 0, "min": 0}
    for name in list(req) + ["reference"]:
        assert len({**req, **opt}[name][1]["tooltip"]) > 20, name
    for word in ("grain", "outside the mask", "reference", "last", "multiband blend"):
        assert word in node.DESCRIPTION, word
    assert node.RETURN_TYPES == ("IMAGE",) and node.FUNCTION == "match" and callable(getattr(node, node.FUNCTION))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            node().match(torch.zeros(1, 16, 16, 3), torch.zeros(1, 16, 16))
