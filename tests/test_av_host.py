"""AV encode / decode nodes and the audio merge, checked on the host (no GPU): the four nodes' schemas against the reference's
(tests/golden/av_schemas.npz), the host plan of lp_audio_merge (crossfade width, mask normalisation, channel / batch
decisions) against the reference's recorded merges (tests/golden/av_merge_*.npz), the prefix-table algorithm the kernel
runs, restated in float64, lp_audio_merge's argument checks, and the errors raised without the ComfyUI runtime."""
import ctypes
import glob
import json
import os
import sys

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, audio, av_nodes, interp_rule
from oracle import lanpaint_oracle as orc
from tests import audio_ref, av_stubs
from tests.audio_ref import RULE_NAMES, fixture_id, host_rule, load_fixture as load, restated_merge, weights_f64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MERGE_FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "av_merge_*.npz")))


# ---------------------------------------------------------------- float64 restatement of what lp_audio_merge computes
def test_fixtures_are_present():
    names = {fixture_id(p) for p in MERGE_FIXTURES}
    assert len(names) >= 12 and {"hard_even_cf", "per_sample_odd_cf", "cf_ge_n", "tie_2_to_41", "err_channels"} <= names
    assert os.path.exists(os.path.join(GOLDEN, "av_schemas.npz")) and os.path.exists(os.path.join(GOLDEN, "av_nodes.npz"))


# ---------------------------------------------------------------- schemas
def _strip_tooltips(input_types):
    return {sect: {name: [spec[0]] + [{k: v for k, v in opt.items() if k != "tooltip"} for opt in spec[1:]]
                   for name, spec in fields.items()}
            for sect, fields in input_types.items()}


def test_node_schemas_match_the_reference():
    ref = json.loads(str(np.load(os.path.join(GOLDEN, "av_schemas.npz"))["schema"]))
    assert set(ref) <= set(av_nodes.NODE_CLASS_MAPPINGS)
    for name, want in ref.items():
        cls = av_nodes.NODE_CLASS_MAPPINGS[name]
        got = json.loads(json.dumps(cls.INPUT_TYPES()))                  # tuples -> lists, as recorded
        assert _strip_tooltips(got) == _strip_tooltips(want["input_types"]), name
        assert list(cls.RETURN_TYPES) == want["return_types"] and list(cls.RETURN_NAMES) == want["return_names"], name
        assert cls.FUNCTION == want["function"] and cls.CATEGORY == want["category"], name
        assert av_nodes.NODE_DISPLAY_NAME_MAPPINGS[name] == want["display_name"]


def test_input_order_matches_the_reference():
    """ComfyUI maps a saved workflow's widget values by position: the order of the inputs matters, not only the set."""
    ref = json.loads(str(np.load(os.path.join(GOLDEN, "av_schemas.npz"))["schema"]))
    order = {"LanPaint_AVDecode": ["samples", "video", "vae", "audio_vae", "mask", "audio_mask", "blend_overlap",
                                   "audio_crossfade"],
             "LanPaint_AVEncode": ["video", "vae", "audio_vae", "mask", "audio_mask"],
             "LanPaint_MiniMaxAudioEncode": ["audio", "vae"], "LanPaint_MiniMaxAudioDecode": ["samples", "vae"]}
    for name, names in order.items():
        assert list(av_nodes.NODE_CLASS_MAPPINGS[name].INPUT_TYPES()["required"]) == names
        assert sorted(ref[name]["input_types"]["required"]) == sorted(names)


# ---------------------------------------------------------------- host plan
@pytest.mark.parametrize("shape", [(7,), (7, 1), (1, 1, 7, 1)])
def test_mask_normalisation(shape):
    m = torch.arange(7, dtype=torch.float64).reshape(shape)
    got = audio.normalize_mask(m)
    assert got.shape == (7,) and got.dtype == torch.float32 and torch.equal(got, torch.arange(7, dtype=torch.float32))


@pytest.mark.parametrize("shape", [(1, 7), (2, 7, 1), (1, 2, 7, 1), (0,)])
def test_mask_normalisation_rejects_other_forms(shape):
    with pytest.raises(ValueError):
        audio.normalize_mask(torch.zeros(shape))


@pytest.mark.parametrize("crossfade,sr,cf", [(0.02, 44100, 882), (0.02, 48000, 960), (1.0, 48000, 48000), (0.02, 2205, 44),
                                             (1.0 / 800, 800, 1), (0.0, 48000, 0), (0.02, 0, 0), (-0.1, 48000, 0),
                                             (1e-9, 48000, 1), (0.015, 1000, 15)])
def test_crossfade_width(crossfade, sr, cf):
    assert audio.crossfade_samples(crossfade, sr) == cf


@pytest.mark.parametrize("path", MERGE_FIXTURES, ids=fixture_id)
def test_plan_against_the_reference(path):
    rec = load(path)
    o, p = torch.from_numpy(rec["orig"]), torch.from_numpy(rec["inpainted"])
    if "error" in rec and fixture_id(path) in ("err_channels", "err_batch"):
        assert str(rec["error"]) == "RuntimeError"
        with pytest.raises(RuntimeError):
            audio.plan_merge(o, p, torch.ones(4), 0, 0)
        return
    if "error" in rec:
        return
    n = min(o.shape[-1], p.shape[-1])
    o, p = o[..., :n], p[..., :n]
    am = audio.normalize_mask(torch.from_numpy(rec["mask"]))
    plan = audio.plan_merge(o, p, am, 0, 0)
    assert (plan.batch, plan.channels, plan.n) == rec["out"].shape
    assert plan.mask_len == am.shape[0]
    # a broadcast operand reads one row through a zero stride; the others step by their own strides
    assert plan.orig_strides[1] == (0 if o.shape[1] == 1 else o.stride(1))
    assert plan.inp_strides[1] == (0 if p.shape[1] == 1 else p.stride(1))
    assert plan.orig_strides[0] == (0 if o.shape[0] == 1 else o.stride(0))
    assert plan.inp_strides[0] == (0 if p.shape[0] == 1 else p.stride(0))


def test_truncated_views_keep_their_row_strides():
    """orig[..., :n] of a longer waveform is merged in place: its channel stride stays the original length."""
    o, p = torch.zeros(1, 2, 640), torch.zeros(1, 2, 611)
    plan = audio.plan_merge(o[..., :611], p, torch.ones(5), 25, 0)
    assert plan.orig_strides == (0, 640) and plan.inp_strides == (0, 611) and plan.n == 611


@pytest.mark.parametrize("path", [p for p in MERGE_FIXTURES if "err_" not in p], ids=fixture_id)
def test_float64_restatement_matches_the_reference(path):
    """The restated arithmetic (the kernel's) against the reference's conv1d: w' within 3e-5 (conv1d sums cf rounded terms)."""
    rec = load(path)
    out, w = restated_merge(rec, host_rule(rec))
    np.testing.assert_allclose(w, rec["weights"], rtol=0, atol=3e-5)
    np.testing.assert_allclose(out, rec["out"], rtol=0, atol=1e-4)
    if float(rec["crossfade"]) == 0.0 or audio.crossfade_samples(float(rec["crossfade"]), int(rec["orig_sr"])) == 1:
        np.testing.assert_array_equal(w, rec["weights"])              # no conv1d: bit for bit
        np.testing.assert_array_equal(out, rec["out"])


@pytest.mark.parametrize("fm,n,cf", [(2, 41, 4), (10, 882, 44), (12, 600, 25), (50, 37, 5), (9, 480, 3), (6, 300, 500),
                                     (30, 48000, 960), (7, 1001, 1), (1025, 2053, 44), (2049, 1500, 45),
                                     (3000, 3000, 961)])
@pytest.mark.parametrize("rule", sorted(RULE_NAMES))
def test_segment_prefix_tables_give_the_window_sums(fm, n, cf, rule):
    """The algorithm of csrc/audio_kernel.hip: start[s] = first sample whose source index is >= s, P[s] = sum over the
    segments before s of mask * length, C(j) = P[src(j)] + mask[src(j)] * (j - start[src(j)]); the window sum as two
    clamped end terms plus C(hi) - C(lo).  Restated here, it equals the plain cumulative sum of the up-sampled mask."""
    rng = np.random.default_rng(fm * 1000 + n)
    am = rng.random(fm, dtype=np.float32)
    src = orc.nearest_exact_src_index(n, fm, RULE_NAMES[rule])
    assert np.all(np.diff(src) >= 0)                                    # monotone: every segment is one run of samples
    start = np.searchsorted(src, np.arange(fm + 1), side="left")
    assert start[0] == 0 and start[fm] == n
    P = np.concatenate([[0.0], np.cumsum(am.astype(np.float64) * np.diff(start))])
    j = np.arange(n + 1)
    s = np.minimum(src[np.minimum(j, n - 1)], fm - 1)
    C = np.where(j >= n, P[fm], P[s] + am[s].astype(np.float64) * (j - start[s]))
    np.testing.assert_allclose(C, np.concatenate([[0.0], np.cumsum(am[src].astype(np.float64))]), rtol=0, atol=1e-9)
    if cf > 1:
        i = np.arange(n)
        lo_raw = i - cf // 2
        lo, hi = np.maximum(lo_raw, 0), np.minimum(lo_raw + cf, n)
        S = (lo - lo_raw) * float(am[src[0]]) + (lo_raw + cf - hi) * float(am[src[-1]]) + C[hi] - C[lo]
        direct = np.array([am[src[np.clip(k - cf // 2 + np.arange(cf), 0, n - 1)]].astype(np.float64).sum() for k in i])
        np.testing.assert_allclose(S, direct, rtol=0, atol=1e-9)


# ---------------------------------------------------------------- the live reference of the GPU shape tests (tests/audio_ref.py)
@pytest.mark.parametrize("path", [p for p in MERGE_FIXTURES if "err_" not in p], ids=fixture_id)
def test_live_reference_matches_the_fixtures(path):
    """tests/audio_ref.py -- torch's own index, int64 counts or direct float64 window sums, no whole-signal prefix -- against
    what the reference recorded and against the float64 restatement: the two references of the GPU tests agree here."""
    rec = load(path)
    o, p = rec["orig"], rec["inpainted"]
    n = min(o.shape[-1], p.shape[-1])
    am = audio.normalize_mask(torch.from_numpy(rec["mask"])).numpy()
    cf = audio.crossfade_samples(float(rec["crossfade"]), int(rec["orig_sr"]))
    src = audio_ref.src_index_live(am.shape[0], n, "cpu")
    w = audio_ref.weights_ref(am, src, cf)
    assert w.dtype == np.float32 and w.shape == (n,)
    np.testing.assert_allclose(w, rec["weights"], rtol=0, atol=3e-5)
    if cf <= 1:
        np.testing.assert_array_equal(w, rec["weights"])
    restated = weights_f64(am, n, cf, host_rule(rec))
    bound = audio_ref.weight_bound(am, src, cf)
    assert np.all(np.abs(w.astype(np.float64) - restated.astype(np.float64)) <= audio_ref.ulp32(w) + bound)
    if audio_ref.is_hard(am):
        assert bound == 0.0
    out = audio_ref.merge_ref(o[..., :n], p[..., :n], w)
    assert out.shape == rec["out"].shape
    np.testing.assert_allclose(out, rec["out"], rtol=0, atol=1e-4)


@pytest.mark.parametrize("fm,n", [(1025, 2053), (2049, 1500), (5000, 37), (250, 480000), (2047, 14329), (7, 2 ** 24 + 12)])
def test_live_source_index_is_the_rule_interp_rule_picks(fm, n):
    """torch's CPU kernel asked directly (interpolating an arange) gives the index of the rule `interp_rule.rule_for` names
    for that call, monotone and inside the mask -- also where float(i) is inexact."""
    src = audio_ref.src_index_live(fm, n, "cpu")
    am = torch.zeros(fm)
    rule = interp_rule.rule_for(am, am.reshape(1, 1, -1), (n,))
    np.testing.assert_array_equal(src, orc.nearest_exact_src_index(n, fm, RULE_NAMES[rule]))
    assert src.dtype == np.int64 and src.shape == (n,) and src[0] >= 0 and src[-1] <= fm - 1 and np.all(np.diff(src) >= 0)
    if n >= fm:
        assert src[0] == 0 and src[-1] == fm - 1 and np.all(np.diff(src) <= 1)            # up-sampled: no segment is empty
    np.testing.assert_array_equal(audio_ref.src_index_live(9, 9, "cpu"), np.arange(9))


@pytest.mark.parametrize("fm,n,cf", [(5, 23, 4), (9, 40, 7), (6, 11, 30), (40, 40, 5), (12, 7, 3)])
def test_reference_window_sums_against_a_plain_loop(fm, n, cf):
    """weights_ref's two ways of summing (int64 counts, float64 conv1d) against the header's formula as a loop with an exactly
    rounded sum; on a 0/1 mask the float64 way, forced, gives the bits of the int64 way."""
    import math
    rng = np.random.default_rng(fm * n + cf)
    src = audio_ref.src_index_live(fm, n, "cpu")
    tap = np.float64(np.float32(1) / np.float32(cf))
    for am in ((rng.random(fm) < 0.5).astype(np.float32), rng.random(fm, dtype=np.float32)):
        w = am[src].astype(np.float64)
        want = np.array([math.fsum(w[min(max(i - cf // 2 + k, 0), n - 1)] for k in range(cf)) * tap for i in range(n)])
        got = audio_ref.weights_ref(am, src, cf)
        if audio_ref.is_hard(am):
            np.testing.assert_array_equal(got, want.astype(np.float32))
            nudged = am.copy()
            nudged[0] = nudged[0] + np.float32(2.0 ** -30) if nudged[0] == 0 else nudged[0]        # soft path, same sums to 1e-9
            assert not audio_ref.is_hard(nudged) or nudged[0] == 1
            np.testing.assert_allclose(audio_ref.weights_ref(nudged, src, cf), got, rtol=0, atol=1e-8)
        else:
            assert np.all(np.abs(got.astype(np.float64) - want) <= audio_ref.ulp32(got))
            assert 0 < audio_ref.weight_bound(am, src, cf) < 1e-12
    assert audio_ref.weights_ref(np.full(3, 0.5, np.float32), np.zeros(10 ** 6, np.int64), 501) is None      # n * cf > 5e8


# ---------------------------------------------------------------- lp_audio_merge argument checks (no device call)
def _desc(**kw):
    d = _cabi.LpAudioDesc()
    d.n, d.mask_len, d.batch, d.channels, d.cf, d.nn_rule = 100, 4, 1, 2, 0, 0
    d.orig_sc = d.inp_sc = 100
    d.mask = d.orig = d.inpainted = d.out = 0x1000
    for k, v in kw.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("bad", [dict(n=0), dict(n=-5), dict(mask_len=0), dict(batch=0), dict(channels=0), dict(cf=-1),
                                 dict(nn_rule=3), dict(nn_rule=-1), dict(orig_sb=-1), dict(inp_sc=-4), dict(mask=None),
                                 dict(orig=None), dict(inpainted=None), dict(out=None), dict(cf=2, workspace=None),
                                 dict(cf=882, workspace=0x1004), dict(mask_len=2**31 - 1)])
def test_lp_audio_merge_rejects_bad_arguments(hip_lib, bad):
    assert hip_lib.lp_audio_merge(ctypes.byref(_desc(**bad)), None) == _cabi.LP_E_INVALID
    assert hip_lib.lp_audio_merge(None, None) == _cabi.LP_E_INVALID


def test_workspace_size_mirrors_the_header():
    src = open(os.path.join(ROOT, "include", "lanpaint_hip.h")).read()
    assert "#define LP_AUDIO_WS_BYTES(mask_len) (12 * ((int64_t)(mask_len) + 1))" in src
    assert _cabi.lp_audio_ws_bytes(10) == 132 and ctypes.sizeof(_cabi.LpAudioDesc) == 24 + 32 + 40


# ---------------------------------------------------------------- errors
def test_rate_mismatch_without_torchaudio(monkeypatch):
    rec = load(os.path.join(GOLDEN, "av_merge_err_rates_no_torchaudio.npz"))
    assert str(rec["error"]) == "RuntimeError"
    monkeypatch.setattr(audio, "torchaudio", None)
    with pytest.raises(RuntimeError, match="torchaudio"):
        audio.merge_audio_with_mask(torch.from_numpy(rec["orig"]), torch.from_numpy(rec["inpainted"]),
                                    torch.from_numpy(rec["mask"]), float(rec["crossfade"]), int(rec["orig_sr"]),
                                    int(rec["result_sr"]))


@pytest.mark.parametrize("name", ["err_channels", "err_batch"])
def test_unbroadcastable_waveforms_raise_what_the_reference_raises(name):
    rec = load(os.path.join(GOLDEN, f"av_merge_{name}.npz"))
    with pytest.raises(RuntimeError):                                   # checked before anything touches a device
        audio.merge_audio_with_mask(torch.from_numpy(rec["orig"]), torch.from_numpy(rec["inpainted"]),
                                    torch.from_numpy(rec["mask"]), float(rec["crossfade"]), int(rec["orig_sr"]),
                                    int(rec["result_sr"]))
    assert str(rec["error"]) == "RuntimeError"


def test_the_4d_mask_the_reference_rejects_is_accepted():
    rec = load(os.path.join(GOLDEN, "av_merge_err_mask_4d.npz"))
    assert str(rec["error"]) == "ValueError" and rec["mask"].shape == (1, 1, 4, 1)
    assert torch.equal(audio.normalize_mask(torch.from_numpy(rec["mask"])), torch.from_numpy(rec["mask"][0, 0, :, 0]))


def test_audio_encode_needs_torchaudio_to_resample(monkeypatch):
    monkeypatch.setattr(audio, "torchaudio", None)
    with pytest.raises(RuntimeError, match="torchaudio"):
        av_nodes.LanPaint_MiniMaxAudioEncode().encode({"waveform": torch.zeros(1, 2, 64), "sample_rate": 44100},
                                                      av_stubs.StubAudioVAE())


def test_nodes_without_the_comfy_runtime(monkeypatch):
    for name in ("comfy", "comfy.nested_tensor", "comfy_api", "comfy_api.latest", "comfy_api.latest._input_impl",
                 "comfy_api.latest._input_impl.video_types", "comfy_api.latest._util", "comfy_api.latest._util.video_types"):
        monkeypatch.setitem(sys.modules, name, None)
    video, mask, audio_mask = av_stubs.node_inputs()
    with pytest.raises(RuntimeError, match="comfy.nested_tensor"):
        av_nodes.LanPaint_AVEncode().encode(video, av_stubs.StubVideoVAE(), av_stubs.StubAudioVAE(), mask, audio_mask)
    with pytest.raises(RuntimeError, match="comfy_api"):
        av_nodes.LanPaint_AVDecode().decode({"samples": None}, video, None, None, mask, audio_mask, 5, 0.02)


# ---------------------------------------------------------------- the encode side runs on the host
def test_av_encode_matches_the_reference():
    rec = load(os.path.join(GOLDEN, "av_nodes.npz"))
    video, mask, audio_mask = av_stubs.node_inputs()
    with av_stubs.comfy_modules():
        latent = av_nodes.LanPaint_AVEncode().encode(video, av_stubs.StubVideoVAE(), av_stubs.StubAudioVAE(), mask,
                                                     audio_mask[:, None])[0]
    zv, za = latent["samples"].unbind()
    mv, ma = latent["noise_mask"].unbind()
    np.testing.assert_array_equal(zv.numpy(), rec["z_video"])
    np.testing.assert_array_equal(za.numpy(), rec["z_audio"])
    np.testing.assert_array_equal(mv.numpy(), rec["noise_mask_video"])
    np.testing.assert_array_equal(ma.numpy(), rec["noise_mask_audio"])
    assert ma.shape == (6,)


def test_av_encode_needs_an_audio_track():
    video, mask, audio_mask = av_stubs.node_inputs()
    video.get_components().audio = None
    with av_stubs.comfy_modules(), pytest.raises(ValueError, match="audio"):
        av_nodes.LanPaint_AVEncode().encode(video, av_stubs.StubVideoVAE(), av_stubs.StubAudioVAE(), mask, audio_mask)


def test_audio_decode_takes_the_audio_stream_and_the_output_rate():
    vae = av_stubs.StubAudioVAE()
    z = torch.ones(1, 2, 8)
    nested = av_stubs.NestedTensor((torch.zeros(1, 3, 2, 4, 4), z))
    a = av_nodes.LanPaint_MiniMaxAudioDecode().decode({"samples": nested}, vae)[0]
    assert a["waveform"].shape == (1, 2, 29) and a["sample_rate"] == 800
    vae.audio_sample_rate_output = 44100
    assert av_nodes.LanPaint_MiniMaxAudioDecode().decode({"samples": z}, vae)[0]["sample_rate"] == 44100

    class Bare:
        def decode(self, z):
            return z.movedim(1, -1)
    assert av_nodes.LanPaint_MiniMaxAudioDecode().decode({"samples": z}, Bare())[0]["sample_rate"] == 32000


def test_audio_encode_upmixes_mono_channels_last():
    seen = {}

    class Spy:
        audio_sample_rate = 800

        def encode(self, x):
            seen["x"] = x
            return x
    av_nodes.LanPaint_MiniMaxAudioEncode().encode({"waveform": torch.arange(12.0).reshape(1, 1, 12), "sample_rate": 800},
                                                  Spy())
    assert seen["x"].shape == (1, 12, 2) and torch.equal(seen["x"][..., 0], seen["x"][..., 1])
