#!/usr/bin/env python3
"""Record the UNMODIFIED reference's AV nodes (src/LanPaint/nodes.py: merge_audio_with_mask :1091-1136, LanPaint_AVEncode
:998-1046, LanPaint_AVDecode :1139-1227, LanPaint_MiniMaxAudioEncode / Decode :811-878) for tests/test_av_host.py and
tests/test_gpu_av_merge.py:

    av_merge_<case>.npz   merge_audio_with_mask on equal-rate inputs: orig, inpainted, mask (the shape handed over),
                          crossfade, orig_sr, result_sr and either `out` plus `weights` -- the crossfaded mask w', recorded as
                          the merge of zeros into ones -- or `error`, the name of the exception the reference raised
    av_schemas.npz        `schema`: JSON of the four nodes' INPUT_TYPES, RETURN_TYPES, RETURN_NAMES, FUNCTION, CATEGORY and
                          display names
    av_nodes.npz          AVEncode and AVDecode run through the stub VAEs of tests/av_stubs.py on its node_inputs()

Run where a checkout of the reference tree is at hand (its root, the directory holding src/LanPaint):
    python tests/golden/make_av_golden.py PATH_TO_REFERENCE
The reference's nodes.py is loaded from its file under a private package name with ComfyUI stubbed; sys.path,
sys.modules and sys.dont_write_bytecode are restored afterwards.  Nothing of it is copied, only its outputs.
"""
from __future__ import annotations

import contextlib
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import av_stubs  # noqa: E402

PKG = "_lanpaint_reference_av"
NODES = ("LanPaint_MiniMaxAudioEncode", "LanPaint_MiniMaxAudioDecode", "LanPaint_AVEncode", "LanPaint_AVDecode")


def _comfy_extras():
    """The rest of what the reference's nodes.py imports at module level, stubbed as its own tests do."""
    utils = types.ModuleType("comfy.utils")
    utils.repeat_to_batch_size = lambda t, b: t
    samplers = types.ModuleType("comfy.samplers")
    samplers.KSAMPLER = type("KSAMPLER", (), {})
    samplers.KSampler = type("KSampler", (), {"SCHEDULERS": ["karras"]})
    mb = types.ModuleType("comfy.model_base")
    mb.ModelType = types.SimpleNamespace(FLUX="FLUX", FLOW="FLOW")
    mb.WAN22 = type("WAN22", (), {})
    ver = types.ModuleType("comfyui_version")
    ver.__version__ = "0.6.0"
    return [("comfy.utils", utils), ("comfy.samplers", samplers), ("comfy.model_base", mb), ("comfyui_version", ver),
            ("nodes", types.ModuleType("nodes")), ("latent_preview", types.ModuleType("latent_preview"))]


@contextlib.contextmanager
def reference_nodes(ref_root):
    saved_path, saved_flag = list(sys.path), sys.dont_write_bytecode
    sys.dont_write_bytecode = True
    pkg = types.ModuleType(PKG)
    pkg.__path__ = [os.path.join(ref_root, "src", "LanPaint")]
    try:
        with av_stubs.comfy_modules(_comfy_extras()):
            sys.modules[PKG] = pkg
            spec = importlib.util.spec_from_file_location(PKG + ".nodes", os.path.join(pkg.__path__[0], "nodes.py"))
            mod = importlib.util.module_from_spec(spec)
            sys.modules[spec.name] = mod
            spec.loader.exec_module(mod)
            yield mod
    finally:
        for k in [k for k in sys.modules if k == PKG or k.startswith(PKG + ".")]:
            del sys.modules[k]
        sys.path[:] = saved_path
        sys.dont_write_bytecode = saved_flag


def _wave(rng, b, c, n):
    return (0.3 * rng.standard_normal((b, c, n))).astype(np.float32)


def _hard(f, on):
    m = np.zeros(f, np.float32)
    for lo, hi in on:
        m[lo:hi] = 1.0
    return m


def merge_cases():
    """(name, orig, inpainted, mask, crossfade, orig_sr, result_sr); equal rates except where an error is the point."""
    rng = np.random.default_rng(20261016)
    yield "hard_even_cf", _wave(rng, 1, 2, 882), _wave(rng, 1, 2, 882), _hard(10, [(3, 6)]), 0.02, 2205, 2205   # cf 44
    yield "soft_mono_orig", _wave(rng, 1, 1, 600), _wave(rng, 1, 2, 600), rng.random(12, dtype=np.float32), 0.05, 500, 500
    yield "f1_mask_mono_inp", _wave(rng, 1, 2, 701), _wave(rng, 1, 1, 701), _hard(8, [(2, 5)])[:, None], 0.03, 700, 700
    yield "per_sample_odd_cf", _wave(rng, 1, 2, 500), _wave(rng, 1, 2, 500), rng.random(500, dtype=np.float32), 0.015, 1000, 1000
    yield "per_sample_no_cf", _wave(rng, 1, 1, 300), _wave(rng, 1, 1, 300), rng.random(300, dtype=np.float32), 0.0, 1000, 1000
    yield "cf_zero", _wave(rng, 1, 2, 400), _wave(rng, 1, 2, 400), _hard(7, [(1, 2), (4, 6)]), 0.0, 800, 800
    yield "cf_one_sample", _wave(rng, 1, 2, 400), _wave(rng, 1, 2, 400), _hard(7, [(2, 5)]), 1.0 / 800, 800, 800
    yield "cf_ge_n", _wave(rng, 1, 2, 300), _wave(rng, 1, 2, 300), _hard(6, [(2, 3)]), 1.0, 500, 500                # cf 500
    yield "six_channel_orig", _wave(rng, 1, 6, 480), _wave(rng, 1, 2, 480), _hard(9, [(0, 3), (7, 9)]), 0.02, 900, 900
    yield "unequal_lengths", _wave(rng, 1, 2, 640), _wave(rng, 1, 2, 611), _hard(5, [(1, 3)]), 0.025, 1000, 1000
    yield "tie_2_to_41", _wave(rng, 1, 1, 41), _wave(rng, 1, 1, 41), np.array([0.0, 1.0], np.float32), 0.0, 41, 41
    yield "tie_2_to_41_cf", _wave(rng, 1, 2, 41), _wave(rng, 1, 2, 41), np.array([1.0, 0.0], np.float32), 0.1, 41, 41
    yield "down_50_to_37", _wave(rng, 1, 2, 37), _wave(rng, 1, 2, 37), rng.random(50, dtype=np.float32), 0.1, 50, 50
    yield "batch_broadcast", _wave(rng, 2, 2, 333), _wave(rng, 1, 2, 333), _hard(11, [(4, 9)]), 0.02, 300, 300
    # where the reference raises
    yield "err_rates_no_torchaudio", _wave(rng, 1, 2, 200), _wave(rng, 1, 2, 160), _hard(4, [(1, 2)]), 0.02, 1000, 800
    yield "err_channels", _wave(rng, 1, 2, 200), _wave(rng, 1, 6, 200), _hard(4, [(1, 2)]), 0.02, 1000, 1000
    yield "err_batch", _wave(rng, 2, 2, 200), _wave(rng, 3, 2, 200), _hard(4, [(1, 2)]), 0.02, 1000, 1000
    yield "err_mask_4d", _wave(rng, 1, 2, 200), _wave(rng, 1, 2, 200), _hard(4, [(1, 2)])[None, None, :, None], 0.02, 1000, 1000


def record_merge(ref, name, orig, inp, mask, crossfade, orig_sr, result_sr):
    rec = dict(orig=orig, inpainted=inp, mask=mask, crossfade=np.float64(crossfade), orig_sr=np.int64(orig_sr),
               result_sr=np.int64(result_sr))
    t = torch.from_numpy
    try:
        rec["out"] = ref.merge_audio_with_mask(t(orig), t(inp), t(mask), crossfade, orig_sr, result_sr).numpy()
        n = rec["out"].shape[-1]
        rec["weights"] = ref.merge_audio_with_mask(torch.zeros(1, 1, n), torch.ones(1, 1, n), t(mask), crossfade, orig_sr,
                                                   orig_sr)[0, 0].numpy()
    except Exception as e:               # noqa: BLE001  (the type is the record)
        rec["error"] = np.array(type(e).__name__)
    path = os.path.join(HERE, f"av_merge_{name}.npz")
    np.savez_compressed(path, **rec)
    return path


def record_schemas(ref):
    schema = {}
    for name in NODES:
        cls = ref.NODE_CLASS_MAPPINGS[name]
        schema[name] = {"input_types": cls.INPUT_TYPES(), "return_types": list(cls.RETURN_TYPES),
                        "return_names": list(cls.RETURN_NAMES), "function": cls.FUNCTION, "category": cls.CATEGORY,
                        "display_name": ref.NODE_DISPLAY_NAME_MAPPINGS[name]}
    path = os.path.join(HERE, "av_schemas.npz")
    np.savez_compressed(path, schema=np.array(json.dumps(schema, sort_keys=True)))
    return path


def record_nodes(ref):
    video, mask, audio_mask = av_stubs.node_inputs()
    vae, avae = av_stubs.StubVideoVAE(), av_stubs.StubAudioVAE()
    latent = ref.LanPaint_AVEncode().encode(video, vae, avae, mask, audio_mask[:, None])[0]
    zv, za = latent["samples"].unbind()
    mv, ma = latent["noise_mask"].unbind()
    out_video, out_audio = ref.LanPaint_AVDecode().decode(latent, video, vae, avae, mask, audio_mask, 5, 0.02)
    comp = out_video.get_components()
    rec = dict(z_video=zv.numpy(), z_audio=za.numpy(), noise_mask_video=mv.numpy(), noise_mask_audio=ma.numpy(),
               frames=comp.images.numpy(), audio=out_audio["waveform"].numpy(),
               sample_rate=np.int64(out_audio["sample_rate"]), frame_rate=np.int64(comp.frame_rate),
               bit_depth=np.int64(out_video.bit_depth), blend_overlap=np.int64(5), audio_crossfade=np.float64(0.02))
    path = os.path.join(HERE, "av_nodes.npz")
    np.savez_compressed(path, **rec)
    return path


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "src", "LanPaint")):
        raise SystemExit("usage: make_av_golden.py PATH_TO_REFERENCE  (the directory holding src/LanPaint)")
    with reference_nodes(os.path.abspath(sys.argv[1])) as ref:
        if ref.torchaudio is not None:
            raise SystemExit("record without torchaudio: the rate-mismatch case records the reference's missing-torchaudio error")
        paths = [record_merge(ref, *case) for case in merge_cases()]
        paths += [record_schemas(ref), record_nodes(ref)]
    total = 0
    for p in paths:
        total += os.path.getsize(p)
        print(os.path.basename(p), os.path.getsize(p), "bytes")
    print("total", total, "bytes")


if __name__ == "__main__":
    main()
