"""The video mask editor's HIP kernels on the MI355X (lanpaint_amd.videomask, csrc/videomask_kernel.hip): exact squared
distances and centroid sums, the morph against the reference's recorded masks (tests/golden/videomask_*.npz), the Pillow
resize bit for bit on the reference's own uint8 codes, end to end, and the node on PNG keyframes."""
import glob
import os
import sys
import types

import numpy as np
import pytest
import torch

from lanpaint_amd import videomask
from tests.device import DEV
from tests.image_checks import _check_edt, _edt

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "videomask_*.npz")))


def _ids(p):
    return os.path.basename(p)[len("videomask_"):-4]


def test_d2_is_exact_on_random_masks():
    rng = np.random.default_rng(11)
    for h, w in ((37, 53), (64, 64), (5, 130), (129, 7)):
        masks = [(rng.random((h, w)) < p).astype(np.float32) for p in (0.002, 0.05, 0.5, 0.97)]
        masks.append(rng.random((h, w)).astype(np.float32))                # soft values: binarised at 0.5
        _check_edt(masks)


def test_d2_edge_shapes():
    rng = np.random.default_rng(12)
    _check_edt([(rng.random((1, 300)) < 0.02).astype(np.float32), np.eye(1, 300, 150, dtype=np.float32)])
    _check_edt([(rng.random((300, 1)) < 0.02).astype(np.float32), np.ones((300, 1), np.float32)])
    _check_edt([np.zeros((17, 23), np.float32), np.ones((17, 23), np.float32), np.full((17, 23), 0.5, np.float32),
                np.full((17, 23), 0.49, np.float32)])
    _check_edt([np.ones((1, 1), np.float32)])
    _check_edt([np.zeros((1, 1), np.float32)])


def test_d2_single_pixel_2048():
    n, y0, x0 = 2048, 1500, 37
    m = np.zeros((n, n), np.float32)
    m[y0, x0] = 1.0
    d2, sdf, csum = _edt([m])
    yy, xx = np.mgrid[:n, :n]
    want = (yy - y0) ** 2 + (xx - x0) ** 2
    assert np.array_equal(d2[0, 0], want)
    bg = np.zeros((n, n), np.int64)
    bg[y0, x0] = 1
    assert np.array_equal(d2[0, 1], bg)
    assert csum[0].tolist() == [1, y0, x0]
    assert sdf[0, y0, x0] == 1.0 and sdf[0, 0, 0] == -np.sqrt(float(want[0, 0]))


def test_d2_on_a_large_mask_against_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    z = np.load(os.path.join(ROOT, "tests", "golden", "videomask_realistic.npz"))
    keys = z["keys"]
    d2, sdf, csum = _edt(list(keys))
    for k, m in enumerate(keys):
        fg = m >= 0.5
        assert np.array_equal(np.sqrt(d2[k, 0].astype(np.float64)), ndimage.distance_transform_edt(~fg))
        assert np.array_equal(np.sqrt(d2[k, 1].astype(np.float64)), ndimage.distance_transform_edt(fg))


def _plan_for(z):
    keys, indices, count = z["keys"], [int(i) for i in z["indices"]], int(z["count"])
    stack = torch.from_numpy(keys).to(DEV)
    sdf, centroids = None, [None] * len(indices)
    if len(indices) > 1:
        _, sdf, csum = videomask.keyframe_edt(stack)
        centroids = [(sy / n, sx / n) if n else None for n, sy, sx in csum.cpu().tolist()]
    return stack, videomask.frame_plan(indices, count, centroids), sdf


@pytest.mark.parametrize("path", FIXTURES, ids=_ids)
def test_morph_matches_the_reference(path):
    """Within 1 fp32 ulp everywhere, bit-identical on >= 99.999 % of the pixels (the device's fp64 exp is the only source of
    difference); the large fixture holds the reference's uint8 codes: within 1 code, identical on >= 99.999 %."""
    z = np.load(path)
    stack, plan, sdf = _plan_for(z)
    frames = torch.from_numpy(z["frames"]).to(DEV)          # the frames the fixture stores (all but in the large case)
    if "morph" in z:
        got = videomask.morph_frames(stack, plan, sdf)[frames].cpu().numpy()
        want = z["morph"]
        ulp = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert ulp.max() <= 1, ulp.max()
    else:
        got = videomask.morph_frames(stack, plan, sdf, codes=True)[frames].cpu().numpy()
        want = z["morph_codes"]
        assert np.abs(got.astype(np.int16) - want.astype(np.int16)).max() <= 1
    assert got.shape == want.shape
    assert np.mean(got == want) >= 0.99999


@pytest.mark.parametrize("path", [p for p in FIXTURES if "final_codes" in np.load(p)], ids=_ids)
def test_resize_is_bit_exact_on_the_reference_codes(path):
    z = np.load(path)
    codes = z["morph_codes"] if "morph_codes" in z else (z["morph"] * 255).astype(np.uint8)
    out = videomask.resize_codes(torch.from_numpy(codes).to(DEV), tuple(int(v) for v in z["size"])).cpu().numpy()
    want = z["final_codes"]
    assert out.shape == want.shape and out.dtype == np.float32
    assert np.array_equal(out, want.astype(np.float32) / np.float32(255.0))


@pytest.mark.parametrize("path", FIXTURES, ids=_ids)
def test_end_to_end_against_the_reference(path):
    z = np.load(path)
    keyframes = {int(i): k for i, k in zip(z["indices"], z["keys"])}
    size = tuple(int(v) for v in z["size"])
    out = videomask.interpolate_masks(keyframes, int(z["count"]), size=size, device=DEV)
    assert out.device.type == "cuda" and out.dtype == torch.float32 and out.shape[0] == int(z["count"])
    got = out[torch.from_numpy(z["frames"]).to(DEV)].cpu().numpy()
    if "final_codes" in z:
        want = z["final_codes"].astype(np.float32) / np.float32(255.0)
    elif "morph" in z:
        want = z["morph"]
    else:
        want = z["morph_codes"].astype(np.float32) / np.float32(255.0)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1.0 / 255.0 + 1e-7
    assert np.mean(got == want) >= 0.9999


def test_interpolate_masks_accepts_tensors_and_keeps_the_device():
    z = np.load(os.path.join(ROOT, "tests", "golden", "videomask_translate.npz"))
    a = videomask.interpolate_masks({int(i): k for i, k in zip(z["indices"], z["keys"])}, int(z["count"]))
    b = videomask.interpolate_masks({int(i): torch.from_numpy(k).to(DEV) for i, k in zip(z["indices"], z["keys"])},
                                    int(z["count"]), device=DEV)
    assert a.is_cuda and torch.equal(a, b)


def test_node_on_png_keyframes(monkeypatch, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from lanpaint_amd.video_nodes import LanPaint_VideoMaskEditor
    z = np.load(os.path.join(ROOT, "tests", "golden", "videomask_multi_soft_down.npz"))
    names = {}
    for i, k in zip(z["indices"], z["keys"]):
        codes = np.round(k * 255.0).astype(np.uint8)
        if i % 2:                                          # the editor's form: the mask in alpha
            rgba = np.zeros(k.shape + (4,), np.uint8)
            rgba[..., 3] = codes
            Image.fromarray(rgba, "RGBA").save(tmp_path / f"k{i}.png")
        else:
            Image.fromarray(codes, "L").save(tmp_path / f"k{i}.png")
        names[str(int(i))] = f"k{i}.png"
    names["4"] = "missing.png"                             # skipped
    count, (w, h) = int(z["count"]), (int(v) for v in z["size"])

    class Video:
        def __init__(self, path):
            self.path = path

        def get_frame_count(self):
            return count

        def get_dimensions(self):
            return (w, h)

        def get_frame_rate(self):
            return 24.0

    fp = types.ModuleType("folder_paths")
    fp.get_input_directory = lambda: str(tmp_path)
    fp.get_annotated_filepath = lambda name: os.path.join(str(tmp_path), name)
    monkeypatch.setitem(sys.modules, "folder_paths", fp)
    mods = ["comfy_api", "comfy_api.latest", "comfy_api.latest._input_impl", "comfy_api.latest._input_impl.video_types"]
    for n in mods:
        monkeypatch.setitem(sys.modules, n, types.ModuleType(n))
    sys.modules[mods[-1]].VideoFromFile = Video
    import json
    vf, mask, audio = LanPaint_VideoMaskEditor().run("clip.mp4", json.dumps(names), '[{"start": 0.25, "end": 0.5}]')
    assert isinstance(vf, Video)
    assert mask.device.type == "cpu" and mask.shape == (count, h, w) and mask.dtype == torch.float32
    assert audio.device.type == "cpu" and audio.shape == (count,) and audio[6:12].eq(1).all() and audio.sum() == 6
    want = z["final_codes"].astype(np.float32) / np.float32(255.0)
    got = mask.numpy()[z["frames"]]
    assert np.abs(got - want).max() <= 1.0 / 255.0 + 1e-7 and np.mean(got == want) >= 0.9999
