"""The patch form of lp_mask_fill (LP_FILL_PATCH), the parts that need no device: the mode macro and the workspace macros against
their Python twins, the entry's refusals (made before any HIP call), mode 0 left alone, the AUTO levels, the wrapper's and the
node's errors, and what the node promises -- measured on the restatement (tests/patch_fill_ref.py), because the device is held to
the restatement's bits by tests/test_gpu_patch_fill.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, fill
from tests import cabi_header, fill_ref
from tests import patch_fill_ref as pref
from tests.cabi_header import _call, _signed

MODES = [(1, 1, 1, 0), (3, 4, 4, 0), (4, 6, 8, 65535), (2, 3, 5, 32768), (2, 3, 5, 32767), (1, 6, 1, 12345)]
WS_CASES = [(1, 1, 1, 1, 1), (1, 1, 1, 3, 6), (2, 17, 33, 3, 3), (3, 32, 32, 4, 2), (1, 2049, 1, 1, 6), (81, 720, 1280, 3, 4),
            (65535, 32768, 32768, 4, 6)]


@pytest.fixture(scope="module")
def c_values(tmp_path_factory):
    """What gcc makes of the header's macros at MODES and WS_CASES, and of the limits."""
    show = lambda key, expr: 'printf("%s\\t%lld\\n", "{}", (long long)({}));'.format(key, expr)       # noqa: E731
    prog = ["#include <stdio.h>", '#include "lanpaint_hip.h"', "int main(void){"]
    prog += [show(_call("LP_FILL_PATCH", m), _call("LP_FILL_PATCH", m)) for m in MODES]
    for b, h, w, c, L in WS_CASES:
        key = _call("WS", (b, h, w, c, L))
        prog.append(show(key, _call("LP_FILL_PATCH_WS_BYTES", (_cabi.fill_ws_bytes(b, h, w, c), b, h, w, L))))
    prog += [show(n, n) for n in ("LP_FILL_PATCH_MAX_RADIUS", "LP_FILL_PATCH_MAX_LEVELS", "LP_FILL_PATCH_MAX_ITERS",
                                  "LP_FILL_PATCH_MAX_CHANNELS", "LP_FILL_PATCH_TILE", "LP_FILL_PATCH_LEVEL_BYTES(1)",
                                  "LP_FILL_PATCH_LEVEL_BYTES(17)")]
    prog.append("return 0;}")
    tmp = tmp_path_factory.mktemp("patch_fill")
    (tmp / "m.c").write_text("\n".join(prog))
    subprocess.run(["gcc", "-I", os.path.join(cabi_header.ROOT, "include"), str(tmp / "m.c"), "-o", str(tmp / "m")], check=True)
    out = subprocess.run([str(tmp / "m")], check=True, capture_output=True, text=True).stdout
    return {k: int(v) for k, v in (line.split("\t") for line in out.splitlines())}


# ---- the macros ---------------------------------------------------------------------------------------------------------------------
def test_the_mode_macro_and_the_limits_agree_with_their_python_twins(c_values):
    for m in MODES:
        word = _cabi.LP_FILL_PATCH(*m)
        assert word == c_values[_call("LP_FILL_PATCH", m)] == pref.mode_word(*m), m
        assert -(1 << 31) <= word < (1 << 31) and _cabi.LpFillDesc(reserved0=word).reserved0 == word
        u = word & 0xFFFFFFFF
        assert (u & 1, (u >> 1) & 7, (u >> 4) & 15, (u >> 8) & 15, (u >> 12) & 15, u >> 16) == (1, 0, *m)
    assert _cabi.LP_FILL_PATCH(3, 4, 4, 0) == 0x4431 and _cabi.LP_FILL_PATCH(1, 1, 1, 65535) < 0
    for name in ("MAX_RADIUS", "MAX_LEVELS", "MAX_ITERS", "MAX_CHANNELS", "TILE"):
        assert getattr(_cabi, "LP_FILL_PATCH_" + name) == c_values["LP_FILL_PATCH_" + name]
    assert (pref.MAX_RADIUS, pref.MAX_LEVELS, pref.MAX_ITERS, pref.MAX_CHANNELS) == (4, 6, 8, 4) == \
        tuple(getattr(_cabi, "LP_FILL_PATCH_" + n) for n in ("MAX_RADIUS", "MAX_LEVELS", "MAX_ITERS", "MAX_CHANNELS"))


def test_the_workspace_macro_agrees_with_its_mirror_and_the_layout(c_values):
    assert c_values["LP_FILL_PATCH_LEVEL_BYTES(1)"] == 4 * 16 + 2 * 16 and c_values["LP_FILL_PATCH_LEVEL_BYTES(17)"] == 4 * 80 + 2 * 32
    for case in WS_CASES:
        b, h, w, c, L = case
        assert _cabi.fill_patch_ws_bytes(*case) == c_values[_call("WS", case)], case
        layout = _cabi.fill_patch_ws_layout(*case)
        assert len(layout) == L and [(g["h"], g["w"]) for g in layout] == fill_ref.levels(h, w)[:1] + \
            [(-(-h // 2 ** l), -(-w // 2 ** l)) for l in range(1, L)]
        at = _cabi.fill_ws_bytes(b, h, w, c)                           # the push-pull part comes first
        for g in layout:
            n = b * g["h"] * g["w"]
            for name, size in (("codes", 4), ("work", 4), ("nnf", 4), ("nnf2", 4), ("hole", 1), ("sets", 1)):
                assert g[name] == at and at % 16 == 0, (case, name)
                at += (n * size + 15) // 16 * 16
        assert at == _cabi.fill_patch_ws_bytes(*case)
    # the levels halve like the push-pull pyramid's
    assert _cabi.fill_patch_levels(720, 1280, 6) == fill_ref.levels(720, 1280)[:6] and _cabi.fill_patch_levels(1, 7, 6)[-1] == (1, 1)
    # 81 frames of 720p at four levels: 24 bytes a pixel, 28 with the push-pull part, about 2 GB
    per_pixel = _cabi.fill_patch_ws_bytes(81, 720, 1280, 3, 4) / (81 * 720 * 1280)
    assert 25 <= per_pixel <= 30


# ---- the entry's refusals -----------------------------------------------------------------------------------------------------------------
def _good(hip_lib, mode, **change):
    p, q = ctypes.c_void_p(256), ctypes.c_void_p(512)                  # never dereferenced: validation comes before any HIP call
    u = mode & 0xFFFFFFFF
    levels = min(max((u >> 8) & 15, 1), 6)
    d = dict(batch=2, height=40, width=150, channels=3, mask_batch=1, reserved0=mode, image=p, mask=p, out=q, ws=p,
             ws_bytes=_cabi.fill_patch_ws_bytes(2, 40, 150, 3, levels))
    d.update(change)
    return hip_lib.lp_mask_fill(ctypes.byref(_cabi.LpFillDesc(**d)), None)


def test_the_patch_form_refuses_a_bad_mode_word_without_a_device(hip_lib):
    E, U, A = _cabi.LP_E_INVALID, _cabi.LP_E_UNSUPPORTED, _cabi.LP_E_ALIGN
    M = _cabi.LP_FILL_PATCH
    good = M(2, 3, 4, 7)
    # every bad field: 0 and one above the limit (a field is four bits wide, so 15 too)
    for bad in (M(0, 3, 4, 7), M(5, 3, 4, 7), M(15, 3, 4, 7), M(2, 0, 4, 7), M(2, 7, 4, 7), M(2, 15, 4, 7), M(2, 3, 0, 7),
                M(2, 3, 9, 7), M(2, 3, 15, 7)):
        assert _good(hip_lib, bad) == E, hex(bad & 0xFFFFFFFF)
    # stray bits: 1, 2 and 3 next to a good word, and any bit with bit 0 clear
    for bit in (1, 2, 3):
        assert _good(hip_lib, good | (1 << bit)) == E, bit
    for bit in range(1, 32):
        assert _good(hip_lib, _signed(1 << bit)) == E, bit
    assert _good(hip_lib, good & ~1) == E
    # C = 5: unsupported in the patch form (with its own workspace, so that nothing else is wrong), fine in mode 0
    ws5 = _cabi.fill_patch_ws_bytes(2, 40, 150, 5, 3)
    assert _good(hip_lib, good, channels=5, ws_bytes=ws5) == U
    assert _good(hip_lib, good, channels=64, ws_bytes=1 << 40) == U
    # a workspace one byte short, for every level count; the push-pull form's size is far too small
    for L in range(1, 7):
        need = _cabi.fill_patch_ws_bytes(2, 40, 150, 3, L)
        assert _good(hip_lib, M(2, L, 4, 7), ws_bytes=need - 1) == E, L
        assert _good(hip_lib, M(2, L, 4, 7), ws_bytes=_cabi.fill_ws_bytes(2, 40, 150, 3)) == E, L
    # the checks of the plain form hold in the patch form too
    for change in ({"batch": 0}, {"height": 0}, {"width": _cabi.LP_DETAIL_MAX_SIDE + 1}, {"channels": 0}, {"mask_batch": 3},
                   {"image": None}, {"mask": None}, {"out": None}, {"ws": None}, {"out": ctypes.c_void_p(256)}):
        assert _good(hip_lib, good, **change) == E, change
    assert _good(hip_lib, good, ws=260) == A
    assert _good(hip_lib, good, batch=65536, ws_bytes=1 << 50) == U


def test_mode_zero_is_the_push_pull_form_with_its_own_workspace(hip_lib):
    """reserved0 = 0 asks for lp_fill_ws_bytes and no more: with one byte less it is refused, and C = 5 is no refusal there (the
    next check, the alignment of ws, answers)."""
    E, A = _cabi.LP_E_INVALID, _cabi.LP_E_ALIGN
    ws = _cabi.fill_ws_bytes(2, 40, 150, 3)
    assert _good(hip_lib, 0, ws_bytes=ws - 1) == E
    assert _good(hip_lib, 0, ws_bytes=ws, ws=260) == A
    assert _good(hip_lib, 0, channels=5, ws_bytes=_cabi.fill_ws_bytes(2, 40, 150, 5), ws=260) == A
    assert hip_lib.lp_fill_ws_bytes(2, 40, 150, 3) == ws                 # lp_fill_ws_bytes stays the push-pull form's


# ---- the wrapper and the node ---------------------------------------------------------------------------------------------------------------
def test_auto_levels():
    # the largest L in 1..6 with min(h_{L-1}, w_{L-1}) >= 4 (2 r + 1), at least 1
    assert fill.patch_levels(720, 1280, 3) == 5                        # 720 -> 360 -> 180 -> 90 -> 45 >= 28 > 23
    assert fill.patch_levels(1024, 1024, 3) == 6                       # 32 >= 28
    assert fill.patch_levels(1024, 1024, 4) == 5                       # 64 >= 36 > 32
    assert fill.patch_levels(27, 500, 3) == 1 and fill.patch_levels(1, 1, 1) == 1 and fill.patch_levels(28, 28, 3) == 1
    # sides are rounded up: 55 halves to 28, 54 to 27
    assert fill.patch_levels(56, 56, 3) == 2 and fill.patch_levels(55, 56, 3) == 2 and fill.patch_levels(54, 56, 3) == 1
    assert fill.patch_levels(12, 12, 1) == 1
    assert fill.patch_levels(24, 25, 1) == 2 and fill.patch_levels(32768, 32768, 4) == 6
    for h, w, r in ((720, 1280, 3), (64, 96, 2), (40, 56, 2), (5, 5, 2), (130, 200, 1), (23, 24, 1)):
        assert fill.patch_levels(h, w, r) == pref.auto_levels(h, w, r), (h, w, r)
    assert fill.AUTO == 0


def test_the_wrapper_refuses_cpu_tensors_and_bad_arguments():
    img, mask = torch.zeros(2, 16, 16, 3), torch.zeros(2, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fill.fill_masked_patch(img, mask)

    class OnDevice(torch.Tensor):                                      # passes require_hip; the checks below come before any device work
        is_cuda = True

    dev_img = torch.zeros(2, 16, 16, 3).as_subclass(OnDevice)
    for bad in (dict(radius=0), dict(radius=5), dict(radius=2.0), dict(radius=True), dict(levels=-1), dict(levels=7), dict(iters=0),
                dict(iters=9), dict(seed=-1), dict(seed=65536), dict(seed=1.5)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            fill.fill_masked_patch(dev_img, mask, **bad)
    with pytest.raises(ValueError, match="at most 4 channels"):
        fill.fill_masked_patch(torch.zeros(1, 8, 8, 5).as_subclass(OnDevice), mask)
    with pytest.raises(ValueError, match=r"\[B, H, W, C\]"):
        fill.fill_masked_patch(torch.zeros(8, 8, 3).as_subclass(OnDevice), mask)
    assert fill.WS_CAP_BYTES == 1 << 30


def test_the_node_keeps_the_protocol_and_has_no_cpu_fallback():
    from lanpaint_amd import fill_patch_nodes as mod
    node = mod.LanPaint_MaskFillPatch
    assert mod.NODE_CLASS_MAPPINGS == {"LanPaint_MaskFillPatch": node}
    assert mod.NODE_DISPLAY_NAME_MAPPINGS == {"LanPaint_MaskFillPatch": "LanPaint Mask Fill (Patch)"}
    req = node.INPUT_TYPES()["required"]
    assert list(req) == ["image", "mask", "radius", "levels", "iters", "seed"]
    assert req["image"][0] == "IMAGE" and req["mask"][0] == "MASK"
    for name, default, lo, hi in (("radius", 3, 1, 4), ("levels", 0, 0, 6), ("iters", 4, 1, 8), ("seed", 0, 0, 65535)):
        assert req[name][0] == "INT" and req[name][1] == {**req[name][1], "default": default, "min": lo, "max": hi}, name
    assert node.RETURN_TYPES == ("IMAGE",) and node.RETURN_NAMES == ("image",) and node.FUNCTION == "fill" and node.CATEGORY == "image"
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            node().fill(torch.zeros(2, 16, 16, 3), torch.zeros(2, 16, 16))


def test_the_patch_kernels_are_a_source_of_the_build():
    from lanpaint_amd import build
    assert "patch_fill_kernel.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "patch_fill_kernel.hip"))


# ---- the restatement: what the node promises ----------------------------------------------------------------------------------------------------
def _tiled(tile, H, W):
    th, tw, _ = tile.shape
    return np.tile(tile, (-(-H // th), -(-W // tw), 1))[:H, :W]


def _scene(codes, box):
    """(the image with 0.5 under the hole, the mask, the push-pull result's codes) for an image given as codes [H, W, 3]."""
    y0, y1, x0, x1 = box
    img = (codes.astype(np.float32) / np.float32(255)).astype(np.float32)
    mask = np.zeros(img.shape[:2], np.float32)
    mask[y0:y1, x0:x1] = 1.0
    img[y0:y1, x0:x1] = 0.5                                            # the original is hidden from the fill
    return img, mask, pref.codes_of(fill_ref.fill_one(img, mask))


RNG = np.random.default_rng(40)
TILE_A, TILE_B = RNG.integers(13, 243, (5, 7, 3)), RNG.integers(13, 243, (6, 9, 3))
TILE_LOW, TILE_HIGH = RNG.integers(13, 120, (6, 9, 3)), RNG.integers(140, 243, (4, 5, 3))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_a_periodic_texture_is_reconstructed_exactly_where_push_pull_blurs(seed):
    """(a) a random 5 x 7 tile of codes 13..242 repeated over 40 x 56 x 3, hole [13:23, 18:32], r 2, L 2, iters 4: every hole pixel
    equals the hidden original; push-pull is off by more than 8 codes on all 140 (its MAE: 55.4 codes)."""
    codes, box = _tiled(TILE_A, 40, 56), (13, 23, 18, 32)
    img, mask, pp = _scene(codes, box)
    y0, y1, x0, x1 = box
    assert int((np.abs(pp - codes)[y0:y1, x0:x1].max(-1) > 8).sum()) == 140
    out, field, target = pref.fill_one(img, mask, 2, 2, 4, seed)
    assert (pref.codes_of(out) == codes).all()
    assert (out[y0:y1, x0:x1] == (codes.astype(np.float32) / np.float32(255))[y0:y1, x0:x1]).all()
    assert (field[target] >= 0).all() and (field[~target] == -1).all() and target.sum() == 14 * 18


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_a_second_periodic_texture_over_three_levels(seed):
    """(b) a 6 x 9 tile over 64 x 96 x 3, hole [21:37, 32:56], r 2, L 3, iters 3: exact."""
    codes = _tiled(TILE_B, 64, 96)
    img, mask, pp = _scene(codes, (21, 37, 32, 56))
    assert np.abs(pp - codes)[21:37, 32:56].mean() > 40                # 55.1 codes
    out, _, _ = pref.fill_one(img, mask, 2, 3, 3, seed)
    assert (pref.codes_of(out) == codes).all()


@pytest.mark.parametrize("seed", [0, 1])
def test_two_textures_meet_under_the_hole(seed):
    """(c) a 6 x 9 tile of codes 13..119 left of x = 48 and a 4 x 5 tile of codes 140..242 right of it on 64 x 96 x 3, hole
    [20:44, 36:60], r 2, L 3, iters 5.  With these tiles seeds 0 and 1 are exact and push-pull's MAE is 31.8 codes; seed 2 leaves
    186 of the 576 hole pixels wrong (MAE 14.1) and is no part of the exact claim."""
    codes = _tiled(TILE_LOW, 64, 96).copy()
    codes[:, 48:] = _tiled(TILE_HIGH, 64, 96)[:, 48:]
    img, mask, pp = _scene(codes, (20, 44, 36, 60))
    pp_mae = np.abs(pp - codes)[20:44, 36:60].mean()
    assert 30 < pp_mae < 34
    out, _, _ = pref.fill_one(img, mask, 2, 3, 5, seed)
    got = pref.codes_of(out)
    assert np.abs(got - codes)[20:44, 36:60].mean() <= pp_mae / 4
    assert (got == codes).all()


def test_the_restatements_consequences():
    """No hole: bit for bit.  No source: the push-pull result bit for bit.  Nothing depends on the image under the mask.  Known
    pixels keep their bits.  A frame's result does not depend on its place in a batch."""
    rng = np.random.default_rng(7)
    img = (np.float32(0.05) + np.float32(0.9) * rng.random((2, 19, 23, 3), dtype=np.float32)).astype(np.float32)
    none = np.zeros((1, 19, 23), np.float32)
    out, field, target = pref.fill_ref_patch(img, none, 2, 2, 2, 3)
    assert (out.view(np.uint32) == img.view(np.uint32)).all() and (field == -1).all() and not target.any()
    speckle = (rng.random((1, 19, 23)) < 0.3).astype(np.float32)
    out, field, _ = pref.fill_ref_patch(img, speckle, 2, 2, 2, 3)
    assert (field == -1).all()                                          # no hole-free 5 x 5 patch
    assert (out.view(np.uint32) == fill_ref.fill_ref(img, speckle).view(np.uint32)).all()
    hole = np.zeros((1, 19, 23), np.float32)
    hole[0, 6:12, 8:15] = 1.0
    hole[0, 0, 0] = np.nan                                             # a NaN is not masked
    out, field, target = pref.fill_ref_patch(img, hole, 1, 2, 3, 5)
    known = ~(hole[0] > 0.5)
    assert known[0, 0] and (out.view(np.uint32)[:, known] == img.view(np.uint32)[:, known]).all()
    assert (field[target] >= 0).all() and (out[:, ~known] != fill_ref.fill_ref(img, hole)[:, ~known]).any()
    poisoned = np.where((hole > 0.5)[..., None], np.float32(np.nan), img).astype(np.float32)
    again, field2, _ = pref.fill_ref_patch(poisoned, hole, 1, 2, 3, 5)
    assert (again.view(np.uint32)[:, ~known] == out.view(np.uint32)[:, ~known]).all() and (field2 == field).all()
    alone, _, _ = pref.fill_ref_patch(img[1:], hole, 1, 2, 3, 5)
    assert (alone.view(np.uint32) == out[1:].view(np.uint32)).all()
    other, _, _ = pref.fill_ref_patch(img, hole, 1, 2, 3, 6)             # the seed matters
    assert (other != out).any()
