"""lp_audio_merge and the AV nodes on the MI355X: every recorded merge of the reference (tests/golden/av_merge_*.npz) through
the kernel, the kernel against the float64 restatement (tests/test_av_host.py), both mask devices on the up-sampling ties,
a 10 s 48 kHz stereo merge against the reference-shaped torch sequence on the device, and AVEncode / AVDecode end to end
through the stub VAEs (tests/golden/av_nodes.npz)."""
import glob
import os

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, audio, av_nodes, interp_rule
from tests import av_stubs
from tests.audio_ref import _reference_sequence, fixture_id, host_rule, lerp_f32, load_fixture as load, restated_merge, weights_f64
from tests.compare import ulps
from tests.device import DEV, _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = [p for p in sorted(glob.glob(os.path.join(GOLDEN, "av_merge_*.npz"))) if "err_" not in p]


def kernel_weights(mask, n, crossfade, sr):
    """w' as the kernel computes it: the merge of zeros into ones."""
    return audio.merge_audio_with_mask(torch.zeros(1, 1, n), torch.ones(1, 1, n), mask, crossfade, sr, sr)[0, 0].cpu().numpy()


def run(rec, mask=None):
    t = torch.from_numpy
    return audio.merge_audio_with_mask(t(rec["orig"]), t(rec["inpainted"]), t(rec["mask"]) if mask is None else mask,
                                       float(rec["crossfade"]), int(rec["orig_sr"]), int(rec["result_sr"]))


@pytest.mark.parametrize("path", FIXTURES, ids=fixture_id)
def test_kernel_matches_the_reference(path):
    rec = load(path)
    out = run(rec)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == rec["out"].shape
    n = rec["out"].shape[-1]
    w = kernel_weights(torch.from_numpy(rec["mask"]), n, float(rec["crossfade"]), int(rec["orig_sr"]))
    np.testing.assert_allclose(w, rec["weights"], rtol=0, atol=3e-5)
    np.testing.assert_allclose(out.cpu().numpy(), rec["out"], rtol=0, atol=1e-4)
    if audio.crossfade_samples(float(rec["crossfade"]), int(rec["orig_sr"])) <= 1:
        np.testing.assert_array_equal(w, rec["weights"])           # no conv1d in the reference: bit for bit
        np.testing.assert_array_equal(out.cpu().numpy(), rec["out"])


@pytest.mark.parametrize("path", FIXTURES, ids=fixture_id)
def test_kernel_matches_the_float64_restatement(path):
    rec = load(path)
    want_out, want_w = restated_merge(rec, host_rule(rec))
    n = want_w.shape[0]
    w = kernel_weights(torch.from_numpy(rec["mask"]), n, float(rec["crossfade"]), int(rec["orig_sr"]))
    assert ulps(w, want_w).max() <= 2
    out = run(rec).cpu().numpy()
    # the blend itself is exact fp32 arithmetic on the kernel's own w'
    o, p = rec["orig"][..., :n], rec["inpainted"][..., :n]
    if o.shape[1] != p.shape[1] and o.shape[1] != 1 and p.shape[1] != 1:
        o = o[:, :p.shape[1]]
    np.testing.assert_array_equal(out, lerp_f32(o, p, w[None, None]))
    assert out.shape == want_out.shape


@pytest.mark.parametrize("fm,n,crossfade,sr", [(2, 41, 0.0, 41), (2, 41, 0.1, 41), (3, 101, 0.0, 101), (14, 201, 0.05, 201),
                                               (7, 1000, 0.004, 1000)])
def test_both_mask_devices(fm, n, crossfade, sr):
    """The reference up-samples on the mask's device: a host mask follows torch's CPU rule, a device mask the GPU rule, and
    the two differ on ties (2 -> 41 at sample 20)."""
    am = torch.from_numpy(np.random.default_rng(fm + n).random(fm, dtype=np.float32))
    cf = audio.crossfade_samples(crossfade, sr)
    w_host = kernel_weights(am, n, crossfade, sr)
    w_dev = kernel_weights(am.to(DEV), n, crossfade, sr)
    assert ulps(w_host, weights_f64(am.numpy(), n, cf, interp_rule.cpu_generic_rule())).max() <= 2
    assert ulps(w_dev, weights_f64(am.numpy(), n, cf, _cabi.LP_NN_ATEN_SCALAR)).max() <= 2
    if cf == 0:                       # torch itself, on each device
        ref = lambda m: torch.nn.functional.interpolate(m[None, None], size=(n,), mode="nearest-exact")[0, 0].cpu().numpy()  # noqa: E731
        np.testing.assert_array_equal(w_host, ref(am))
        np.testing.assert_array_equal(w_dev, ref(am.to(DEV)))
    if (fm, n) == (2, 41) and cf == 0:
        assert w_host[20] != w_dev[20]


def _ten_seconds():
    sr, fps = 48000, 25
    n, fm = 10 * sr, 10 * fps
    g = torch.Generator(device="cpu").manual_seed(5)
    orig = (0.3 * torch.randn(1, 2, n, generator=g)).to(DEV)
    inp = (0.3 * torch.randn(1, 2, n, generator=g)).to(DEV)
    am = torch.zeros(fm)
    am[40:90] = 1.0
    am[130:131] = 1.0
    am[200:] = 1.0
    return orig, inp, am.to(DEV), n, sr


def test_ten_seconds_48k_stereo_against_the_torch_sequence():
    orig, inp, am, n, sr = _ten_seconds()
    crossfade = 0.02
    want, want_w = _reference_sequence(orig, inp, am, crossfade, sr)
    got = audio.merge_audio_with_mask(orig, inp, am, crossfade, sr, sr)
    w = kernel_weights(am, n, crossfade, sr)
    np.testing.assert_allclose(w, want_w.cpu().numpy(), rtol=0, atol=3e-5)
    np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=0, atol=1e-4)
    cf = audio.crossfade_samples(crossfade, sr)
    assert ulps(w, weights_f64(am.cpu().numpy(), n, cf, _cabi.LP_NN_ATEN_SCALAR)).max() <= 2


def test_one_second_crossfade_against_the_float64_restatement():
    """cf = 48 000 samples: O(1) per sample in the kernel; the restatement is the reference's window sum done exactly."""
    orig, inp, am, n, sr = _ten_seconds()
    w = kernel_weights(am, n, 1.0, sr)
    want = weights_f64(am.cpu().numpy(), n, 48000, _cabi.LP_NN_ATEN_SCALAR)
    assert ulps(w, want).max() <= 2
    got = audio.merge_audio_with_mask(orig, inp, am, 1.0, sr, sr).cpu().numpy()
    np.testing.assert_array_equal(got, lerp_f32(orig.cpu().numpy(), inp.cpu().numpy(), w[None, None]))


def test_misaligned_rows_take_the_scalar_path():
    """A device view one sample into rows of 1005 (no 16 B alignment): the same values as its contiguous copy, which takes
    the float4 path."""
    g = torch.Generator(device="cpu").manual_seed(9)
    base_o, p = torch.randn(2, 3, 1005, generator=g).to(DEV), torch.randn(1, 1, 1000, generator=g).to(DEV)
    am = torch.tensor([0.0, 1.0, 1.0, 0.0, 0.5])
    view = base_o[..., 1:1001]
    assert view.data_ptr() % 16 != 0 and view.stride(1) == 1005
    a = audio.merge_audio_with_mask(view, p, am, 0.01, 1000, 1000)
    b = audio.merge_audio_with_mask(view.contiguous(), p, am, 0.01, 1000, 1000)
    assert a.shape == (2, 3, 1000)
    torch.testing.assert_close(a, b, rtol=0, atol=0)


def test_the_4d_mask_merges_like_its_flat_form():
    rec = load(os.path.join(GOLDEN, "av_merge_err_mask_4d.npz"))
    a = run(rec)
    b = run(rec, mask=torch.from_numpy(rec["mask"][0, 0, :, 0]))
    torch.testing.assert_close(a, b, rtol=0, atol=0)


def test_av_decode_end_to_end():
    rec = load(os.path.join(GOLDEN, "av_nodes.npz"))
    video, mask, audio_mask = av_stubs.node_inputs()
    vae, avae = av_stubs.StubVideoVAE(), av_stubs.StubAudioVAE()
    with av_stubs.comfy_modules():
        latent = av_nodes.LanPaint_AVEncode().encode(video, vae, avae, mask, audio_mask[:, None])[0]
        out_video, out_audio = av_nodes.LanPaint_AVDecode().decode(latent, video, vae, avae, mask, audio_mask,
                                                                    int(rec["blend_overlap"]), float(rec["audio_crossfade"]))
    comp = out_video.get_components()
    assert comp.images.device.type == "cpu" and out_audio["waveform"].device.type == "cpu"
    np.testing.assert_allclose(comp.images.numpy(), rec["frames"], rtol=0, atol=3e-6)
    np.testing.assert_allclose(out_audio["waveform"].numpy(), rec["audio"], rtol=0, atol=3e-5)
    assert out_audio["sample_rate"] == int(rec["sample_rate"]) and comp.audio is out_audio
    assert comp.frame_rate == int(rec["frame_rate"]) and out_video.bit_depth == int(rec["bit_depth"])


def test_av_decode_without_a_source_audio_track_returns_the_inpainted_audio():
    video, mask, audio_mask = av_stubs.node_inputs()
    vae, avae = av_stubs.StubVideoVAE(), av_stubs.StubAudioVAE()
    with av_stubs.comfy_modules():
        latent = av_nodes.LanPaint_AVEncode().encode(video, vae, avae, mask, audio_mask)[0]
        video.get_components().audio = None
        _, out_audio = av_nodes.LanPaint_AVDecode().decode(latent, video, vae, avae, mask, audio_mask, 5, 0.02)
    want = av_nodes.LanPaint_MiniMaxAudioDecode().decode({"samples": latent["samples"]}, avae)[0]
    torch.testing.assert_close(out_audio["waveform"], want["waveform"], rtol=0, atol=0)
    assert out_audio["sample_rate"] == want["sample_rate"]
