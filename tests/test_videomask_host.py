"""The video mask editor's host side, no GPU needed: widget parsing, the audio-interval rule, the per-frame plan against the
reference's recorded fixtures (tests/golden/videomask_*.npz, tests/golden/make_videomask_golden.py), Pillow's BILINEAR
coefficient tables against live PIL, the new C-ABI entries' argument checks, the node's protocol, and the float64 arbiter of
the device tests (tests/videomask_ref.py) pinned bit for bit to the same fixtures."""
import ctypes
import glob
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, videomask
from lanpaint_amd.videomask import FRAME_DTYPE, frame_plan, parse_keyframes_widget, pillow_bilinear_coeffs
from tests import videomask_ref as vref
from tests.image_inputs import _apply, _pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "videomask_*.npz")))


def _fixture_morph(z):
    return z["morph"] if "morph" in z else z["morph_codes"]


def _centroids(keys):
    out = []
    for k in keys:
        ys, xs = np.where(k >= 0.5)
        out.append((float(ys.mean()), float(xs.mean())) if len(xs) else None)
    return out


# ---- widgets -------------------------------------------------------------------------------------------------------------
def test_parse_keyframes_widget():
    assert parse_keyframes_widget('{"0": "a.png", "12": "b.png"}') == {0: "a.png", 12: "b.png"}
    assert parse_keyframes_widget('{"3": "a.png", "x": "b.png", "4": 5, "5": null, "6": ["c"]}') == {3: "a.png"}
    for bad in ("", None, "{", "not json", "[1, 2]", '"a.png"', "3"):
        assert parse_keyframes_widget(bad) == {}


def test_audio_mask_intervals():
    f = videomask.audio_mask_frames
    assert f("[]", 10, 24.0).tolist() == [0.0] * 10
    m = f(json.dumps([{"start": 0.1, "end": 0.2}]), 10, 24.0)          # floor(2.4) = 2 .. ceil(4.8) = 5
    assert m.dtype == torch.float32 and m.tolist() == [0, 0, 1, 1, 1, 0, 0, 0, 0, 0]
    m = f([{"start": -1.0, "end": 0.05}, {"start": 0.3, "end": 9.0}], 10, 10.0)   # clamped to [0, count)
    assert m.tolist() == [1, 0, 0, 1, 1, 1, 1, 1, 1, 1]
    m = f([{"start": 0.5, "end": 0.5}, {"start": 0.6, "end": 0.2}, {"start": "x"}, 7, None, {"end": 0.15}], 10, 10.0)
    assert m.tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 0, 0]                   # only the last entry (start defaults to 0)
    assert f("{not json", 4, 10.0).tolist() == [0] * 4
    assert f('{"start": 0, "end": 1}', 4, 10.0).tolist() == [0] * 4       # not a list


# ---- the frame plan --------------------------------------------------------------------------------------------------------
def test_frame_dtype_is_the_c_struct():
    assert FRAME_DTYPE.itemsize == ctypes.sizeof(_cabi.LpVmaskFrame)
    for name, _ in _cabi.LpVmaskFrame._fields_:
        assert FRAME_DTYPE.fields[name][1] == getattr(_cabi.LpVmaskFrame, name).offset, name


def test_fixtures_present_and_small():
    names = {os.path.basename(p)[len("videomask_"):-4] for p in FIXTURES}
    assert {"translate", "translate_far", "grow_shrink_full", "multi_soft", "single", "all_beyond", "beyond_end",
            "exact_half", "realistic"} <= names
    assert max(os.path.getsize(p) for p in FIXTURES) < 300_000
    assert sum(os.path.getsize(p) for p in FIXTURES) < 600_000
    for p in FIXTURES:                                     # the large case stores a sample of its frames, the rest all
        z = np.load(p)
        frames = z["frames"].tolist()
        assert frames == sorted(set(frames)) and all(0 <= t < int(z["count"]) for t in frames)
        assert _fixture_morph(z).shape[0] == len(frames)
        if "realistic" not in p:
            assert frames == list(range(int(z["count"])))


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[10:-4])
def test_frame_plan_matches_the_reference(path):
    """Kinds, key indices and the four whole-pixel shifts of every frame against what the reference did: keyframe frames hold
    the painted values, frames outside the window are zero, inner frames got the shifts recorded from its _shift calls."""
    z = np.load(path)
    keys, indices, count = z["keys"], [int(i) for i in z["indices"]], int(z["count"])
    plan = frame_plan(indices, count, _centroids(keys))
    morph, frames = _fixture_morph(z), [int(t) for t in z["frames"]]
    assert plan.shape == (count,) and morph.shape[0] == len(frames)
    inner = np.flatnonzero(plan["kind"] == _cabi.LP_VMASK_INNER)
    assert inner.tolist() == z["inner_frames"].tolist()
    got = np.stack([plan["sy1"], plan["sx1"], -plan["sy2"], -plan["sx2"]], 1)[inner] if len(inner) else np.zeros((0, 4))
    assert np.array_equal(got, z["shifts"])
    for i, t in enumerate(frames):
        p = plan[t]
        if p["kind"] == _cabi.LP_VMASK_KEY:
            want = keys[p["key_lo"]] if "morph" in z else (keys[p["key_lo"]] * 255).astype(np.uint8)
            assert indices[p["key_lo"]] == t and np.array_equal(morph[i], want)
        elif p["kind"] == _cabi.LP_VMASK_ZERO:
            assert not morph[i].any()
        else:
            assert indices[p["key_lo"]] < t < indices[p["key_hi"]] and p["key_hi"] == p["key_lo"] + 1
            assert p["wf"] == (t - indices[p["key_lo"]]) / (indices[p["key_hi"]] - indices[p["key_lo"]])
            assert p["omw"] == 1.0 - p["wf"]


def test_frame_plan_edges():
    assert (frame_plan([7, 9], 5, [None, None])["kind"] == 0).all()                   # no keyframe below count
    p = frame_plan([2], 6, [None])
    assert p["kind"].tolist() == [0, 0, 1, 0, 0, 0]
    p = frame_plan([0, 9], 5, [(1.0, 1.0), (1.0, 10.0)])                              # the reference would raise here
    assert p["kind"].tolist() == [1, 2, 2, 2, 2] and p["sx1"].tolist()[1:] == [1, 2, 3, 4]
    p = frame_plan([0, 4], 5, [None, (3.0, 3.0)])                                     # growth from empty: no shift
    assert not p["sx1"].any() and not p["sy2"].any()


# ---- Pillow's BILINEAR -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", _pairs())
def test_pillow_coefficients_equal_live_pil(src, dst):
    Image = pytest.importorskip("PIL.Image")
    (w, h), (ow, oh) = src, dst
    rng = np.random.default_rng(w * 1000 + h)
    codes = rng.integers(0, 256, (h, w), dtype=np.uint8)
    codes[rng.random((h, w)) < 0.5] = 0                     # masks: flat regions and edges
    bx, kx = pillow_bilinear_coeffs(w, ow)
    by, ky = pillow_bilinear_coeffs(h, oh)
    assert bx.dtype == np.int32 and kx.dtype == np.int32 and (bx[:, 1] <= kx.shape[1]).all()
    want = np.asarray(Image.fromarray(codes).resize((ow, oh), Image.BILINEAR))
    assert np.array_equal(_apply(codes, bx, kx, by, ky), want)


@pytest.mark.parametrize("path", [p for p in FIXTURES if "realistic" not in p and "final_codes" in np.load(p)],
                         ids=lambda p: os.path.basename(p)[10:-4])
def test_pillow_model_reproduces_the_fixture_resize(path):
    z = np.load(path)
    morph, (ow, oh) = z["morph"], [int(v) for v in z["size"]]
    h, w = morph.shape[1:]
    bx, kx = pillow_bilinear_coeffs(w, ow)
    by, ky = pillow_bilinear_coeffs(h, oh)
    for t in range(morph.shape[0]):
        assert np.array_equal(_apply((morph[t] * 255).astype(np.uint8), bx, kx, by, ky), z["final_codes"][t])


# ---- the arbiter of the device tests (tests/videomask_ref.py) ------------------------------------------------------------------
@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[10:-4])
def test_arbiter_reproduces_every_fixture_bit_for_bit(path):
    """morph_ref on this project's frame_plan against what the reference recorded: every fp32 bit of `morph`, every code of
    `morph_codes`.  The arbiter's own error is therefore zero; whatever a device test shows against it is the device's."""
    z = np.load(path)
    keys, indices, count = z["keys"], [int(i) for i in z["indices"]], int(z["count"])
    plan = frame_plan(indices, count, _centroids(keys))[z["frames"]]
    got = vref.morph_ref(keys, plan)
    assert got.dtype == np.float32 and got.shape == _fixture_morph(z).shape
    if "morph" in z:
        assert np.array_equal(got.view(np.uint32), z["morph"].view(np.uint32))
    else:
        assert np.array_equal(vref.codes_ref(got), z["morph_codes"])
    if "final_codes" in z and "realistic" not in path:
        pytest.importorskip("PIL.Image")
        want = z["final_codes"].astype(np.float32) / np.float32(255)
        assert np.array_equal(vref.pil_resize_ref(vref.codes_ref(got), [int(v) for v in z["size"]]), want)


def test_arbiter_codes_of_the_realistic_fixture():
    z = np.load(os.path.join(ROOT, "tests", "golden", "videomask_realistic.npz"))
    keys, indices = z["keys"], [int(i) for i in z["indices"]]
    plan = frame_plan(indices, int(z["count"]), _centroids(keys))[z["frames"]]
    assert (plan["kind"] == _cabi.LP_VMASK_INNER).any()
    codes = vref.codes_ref(vref.morph_ref(keys, plan))
    assert codes.dtype == np.uint8 and np.array_equal(codes, z["morph_codes"])


def test_arbiter_shift():
    f = np.arange(1.0, 13.0).reshape(3, 4)                 # no zero among the values: a vacated pixel is recognisable
    assert np.array_equal(vref.shift_ref(f, 0, 0), f)
    assert np.array_equal(vref.shift_ref(f, 1, 0), [[0, 0, 0, 0], [1, 2, 3, 4], [5, 6, 7, 8]])
    assert np.array_equal(vref.shift_ref(f, -1, 0), [[5, 6, 7, 8], [9, 10, 11, 12], [0, 0, 0, 0]])
    assert np.array_equal(vref.shift_ref(f, 0, 1), [[0, 1, 2, 3], [0, 5, 6, 7], [0, 9, 10, 11]])
    assert np.array_equal(vref.shift_ref(f, 0, -3), [[4, 0, 0, 0], [8, 0, 0, 0], [12, 0, 0, 0]])
    assert np.array_equal(vref.shift_ref(f, 2, -1), [[0, 0, 0, 0], [0, 0, 0, 0], [2, 3, 4, 0]])
    assert np.array_equal(vref.shift_ref(f, -2, 3), [[0, 0, 0, 9], [0, 0, 0, 0], [0, 0, 0, 0]])
    for dy, dx in ((3, 0), (-3, 0), (0, 4), (0, -4), (3, 4), (-3, -4), (100, 1), (1, -100), (-7, 9), (2, 4), (-3, 1)):
        assert not vref.shift_ref(f, dy, dx).any(), (dy, dx)             # past the frame in either direction: all vacated
    out = vref.shift_ref(f, 1, 1)
    assert out.dtype == f.dtype and out is not f and f[0, 0] == 1.0
    g = np.arange(1.0, 6.0).reshape(1, 5)
    assert np.array_equal(vref.shift_ref(g, 0, 2), [[0, 0, 1, 2, 3]]) and not vref.shift_ref(g, 1, 0).any()
    for dy in range(-4, 5):                                # the definition, element by element
        for dx in range(-5, 6):
            out = vref.shift_ref(f, dy, dx)
            for y in range(3):
                for x in range(4):
                    inside = 0 <= y - dy < 3 and 0 <= x - dx < 4
                    assert out[y, x] == (f[y - dy, x - dx] if inside else 0.0)


def test_arbiter_sdf_rules():
    assert np.array_equal(vref.sdf_ref(np.zeros((3, 8), np.float32)), np.full((3, 8), -4.0))
    assert np.array_equal(vref.sdf_ref(np.ones((9, 2), np.float32)), np.full((9, 2), 4.5))
    half, below = np.float32(0.5), np.nextafter(np.float32(0.5), np.float32(0))
    assert np.array_equal(vref.sdf_ref(np.full((2, 2), half)), np.full((2, 2), 1.0))                # 0.5 is foreground
    assert np.array_equal(vref.sdf_ref(np.full((2, 2), below)), np.full((2, 2), -1.0))
    k = np.zeros((1, 5), np.float32)
    k[0, 1:3] = 1.0
    assert vref.sdf_ref(k).tolist() == [[-1.0, 1.0, 1.0, -1.0, -2.0]]
    k = np.zeros((4, 4), np.float32)
    k[0, 0] = 0.75
    assert vref.sdf_ref(k)[3, 3] == -np.sqrt(18.0) and vref.sdf_ref(k)[0, 0] == 1.0


def test_arbiter_own_edt_equals_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(21)
    for h, w in ((1, 1), (1, 40), (40, 1), (17, 23), (64, 64), (31, 200)):
        for p in (0.02, 0.5, 0.98):
            a = rng.random((h, w)) < p
            a.flat[rng.integers(a.size)] = False           # a pixel to measure to
            assert np.array_equal(vref.edt_numpy(a), ndimage.distance_transform_edt(a)), (h, w, p)
    a = np.ones((50, 70), bool)
    a[49, 0] = False
    assert np.array_equal(vref.edt_numpy(a), ndimage.distance_transform_edt(a))
    assert vref.edt_numpy(a)[0, 69] == np.sqrt(49.0 ** 2 + 69.0 ** 2)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_vmask_entries_reject_bad_arguments_without_a_device(hip_lib):
    C, E = ctypes, _cabi.LP_E_INVALID
    p = C.c_void_p(16)                                     # never dereferenced: validation comes before any HIP call
    assert hip_lib.lp_vmask_edt(None, None) == E
    good = dict(n_keys=2, height=8, width=8, keys=p, d2=p, sdf=p, csum=p)
    for change in ({"n_keys": 0}, {"height": 0}, {"width": -3}, {"width": 16385}, {"height": 1 << 20}, {"keys": None},
                   {"d2": None}, {"sdf": None}, {"csum": None}):
        d = _cabi.LpVmaskEdtDesc(**{**good, **change})
        assert hip_lib.lp_vmask_edt(C.byref(d), None) == E, change
    assert hip_lib.lp_vmask_morph(None, None) == E
    good = dict(n_frames=3, n_keys=2, height=8, width=8, flags=0, frames=p, keys=p, sdf=None, out=p)
    for change in ({"n_frames": 0}, {"n_keys": 0}, {"height": 0}, {"width": 16385}, {"frames": None}, {"keys": None},
                   {"out": None}, {"flags": 6}):
        d = _cabi.LpVmaskMorphDesc(**{**good, **change})
        assert hip_lib.lp_vmask_morph(C.byref(d), None) == E, change
    assert hip_lib.lp_vmask_resize(None, None) == E
    good = dict(n_frames=3, in_h=8, in_w=8, out_h=16, out_w=16, ksize_x=3, ksize_y=3, src=p, bounds_x=p, weights_x=p,
                bounds_y=p, weights_y=p, dst=p)
    for change in ({"n_frames": 0}, {"in_h": 0}, {"out_w": 0}, {"out_h": 16385}, {"ksize_x": 0}, {"ksize_y": -1},
                   {"src": None}, {"dst": None}, {"bounds_x": None}, {"weights_y": None}):
        d = _cabi.LpVmaskResizeDesc(**{**good, **change})
        assert hip_lib.lp_vmask_resize(C.byref(d), None) == E, change


# ---- the Python API's argument rules (raised before any device is needed) ----------------------------------------------------
def test_interpolate_masks_rejects_bad_arguments():
    k = np.zeros((4, 5), np.float32)
    with pytest.raises(ValueError):
        videomask.interpolate_masks({0: k}, 0)
    with pytest.raises(ValueError):
        videomask.interpolate_masks({}, 3)
    with pytest.raises(ValueError):
        videomask.interpolate_masks({0: k, 3: np.zeros((5, 4), np.float32)}, 5)
    with pytest.raises(ValueError):
        videomask.interpolate_masks({0: np.zeros((2, 2, 2), np.float32)}, 5)
    with pytest.raises(ValueError):
        videomask.interpolate_masks({0: k}, 5, size=(16385, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        videomask.interpolate_masks({0: k}, 5, device="cpu")


# ---- the node ----------------------------------------------------------------------------------------------------------------
class _Video:
    def __init__(self, path, frames=6, size=(20, 12), fps=None, rate=None):
        self.path, self.frames, self.size, self.fps, self.rate = path, frames, size, fps, rate
        if fps is not None:
            self.get_fps = lambda: self.fps

    def get_frame_count(self):
        return self.frames

    def get_dimensions(self):
        return self.size

    def get_frame_rate(self):
        return self.rate


def _install_comfy(monkeypatch, tmp_path, video_cls):
    fp = types.ModuleType("folder_paths")
    fp.get_input_directory = lambda: str(tmp_path)
    fp.get_annotated_filepath = lambda name: os.path.join(str(tmp_path), name)
    monkeypatch.setitem(sys.modules, "folder_paths", fp)
    names = ["comfy_api", "comfy_api.latest", "comfy_api.latest._input_impl", "comfy_api.latest._input_impl.video_types"]
    for n in names:
        monkeypatch.setitem(sys.modules, n, types.ModuleType(n))
    sys.modules[names[-1]].VideoFromFile = video_cls


def test_node_protocol_and_own_mappings(monkeypatch, tmp_path):
    from lanpaint_amd import nodes, video_nodes
    node = video_nodes.LanPaint_VideoMaskEditor
    assert node.RETURN_TYPES == ("VIDEO", "MASK", "MASK") and node.FUNCTION == "run" and node.CATEGORY == "video"
    req = node.INPUT_TYPES()["required"]
    assert set(req) == {"video", "keyframes", "audio_mask"} and req["video"][1]["video_upload"] is True
    assert req["keyframes"][0] == "STRING" and req["audio_mask"][0] == "STRING"
    assert video_nodes.NODE_CLASS_MAPPINGS == {"LanPaint_VideoMaskEditor": node}
    assert "LanPaint_VideoMaskEditor" not in nodes.NODE_CLASS_MAPPINGS
    (tmp_path / "clip.mp4").write_bytes(b"")
    (tmp_path / "notes.txt").write_bytes(b"")
    _install_comfy(monkeypatch, tmp_path, _Video)
    assert node.INPUT_TYPES()["required"]["video"][0] == ["clip.mp4"]


def test_node_without_keyframes_returns_host_zeros(monkeypatch, tmp_path):
    from fractions import Fraction
    from lanpaint_amd.video_nodes import LanPaint_VideoMaskEditor
    _install_comfy(monkeypatch, tmp_path, lambda path: _Video(path, frames=6, size=(20, 12), rate=Fraction(10, 1)))
    vf, mask, audio = LanPaint_VideoMaskEditor().run("clip.mp4", '{"2": "missing.png"}', '[{"start": 0.1, "end": 0.3}]')
    assert vf.path == os.path.join(str(tmp_path), "clip.mp4")
    assert mask.device.type == "cpu" and mask.shape == (6, 12, 20) and not mask.any()
    assert audio.device.type == "cpu" and audio.tolist() == [0, 1, 1, 0, 0, 0]
    with pytest.raises(ValueError):
        LanPaint_VideoMaskEditor().run("", "{}", "[]")


def test_node_needs_comfy_api(monkeypatch):
    from lanpaint_amd import video_nodes
    monkeypatch.setattr(video_nodes, "_video_from_file", lambda: None)
    with pytest.raises(RuntimeError, match="comfy_api"):
        video_nodes.LanPaint_VideoMaskEditor().run("clip.mp4")
