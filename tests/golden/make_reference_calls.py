#!/usr/bin/env python3
"""Record the UNMODIFIED reference's answers for tests/test_oracle_vs_reference_live.py into two fixtures, so that the
differential tests of the oracle need nothing outside this repository:

    ref_random_calls.npz   engine calls drawn at random (shapes, VE / flow, masks, inner-step counts, hyper-parameters,
                           model-output forms, the inner early stop): inputs, the xi stream the reference consumed, its
                           outputs and its early-stop trace
    ref_reshape_mask.npz   reshape_mask on random ComfyUI mask layouts, both sides of the 0.6.0 gate (SHA-256 digests of
                           the bit-exact outputs), and min_step_frac_effective_steps on a dense grid

Run where a checkout of the reference tree is at hand (its root, the directory holding src/LanPaint):
    python tests/golden/make_reference_calls.py PATH_TO_REFERENCE
The reference is imported, never copied; its torch.randn_like is wrapped, never its source.
"""
from __future__ import annotations

import importlib
import json
import math
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import golden_cases as gc      # noqa: E402  (imported before the reference tree, which has a `tests` package too)

N_CALLS = 80
SHAPES = [(1, 4, 6, 6), (2, 4, 5, 7), (3, 2, 4, 4), (1, 3, 3, 4, 5), (2, 2, 2, 3, 3), (1, 1, 9)]
MASK_KINDS = ["box", "random", "soft", "ones", "zeros"]
FORMS = ["tuple", "list1", "single", "triple"]
STOPS = [None, (3.0, 1), (0.4, 2), (1e-9, 1)]


def call_inputs(shape, flow, mask_kind, row_sigmas, seed):
    """(sigma, x, y, noise, mask) of one engine call, all fp32 numpy, from `seed`."""
    rng = np.random.default_rng(seed)
    b = shape[0]
    base = float(rng.uniform(0.05, 0.95)) if flow else float(np.exp(rng.uniform(np.log(0.03), np.log(14.0))))
    scale = rng.uniform(0.6, 1.0, size=b).astype(np.float32) if (row_sigmas and b > 1) else np.ones(b, np.float32)
    sigma = (np.float32(base) * scale).astype(np.float32)
    y, noise = rng.standard_normal(shape, dtype=np.float32), rng.standard_normal(shape, dtype=np.float32)
    sb = sigma.reshape((-1,) + (1,) * (len(shape) - 1))
    x = (sb * noise + (1 - sb) * y).astype(np.float32) if flow else (y + noise * sb).astype(np.float32)
    mask = {"box": lambda: np.concatenate([np.ones(shape[:-1] + (shape[-1] // 2,), np.float32), np.zeros(shape[:-1] + (shape[-1] - shape[-1] // 2,), np.float32)], -1),
            "random": lambda: (rng.random(shape) > 0.5).astype(np.float32), "soft": lambda: rng.random(shape, dtype=np.float32),
            "ones": lambda: np.ones(shape, np.float32), "zeros": lambda: np.zeros(shape, np.float32)}[mask_kind]()
    return sigma, x, y, noise, mask


# ---------------------------------------------------------------- the reference, imported
def _reference_nodes(ref_root, version):
    """The reference's nodes.py with ComfyUI stubbed the way its own tests stub it (tests/test_reshape_mask.py:18-54)."""
    comfy_mod = types.ModuleType("comfy")
    comfy_mod.__path__ = []
    utils = types.ModuleType("comfy.utils")

    def repeat_to_batch_size(t, b):                       # comfy.utils semantics: narrow when larger, tile + narrow when smaller
        if t.shape[0] > b:
            return t[:b]
        if t.shape[0] < b:
            return t.repeat([math.ceil(b / t.shape[0])] + [1] * (t.ndim - 1))[:b]
        return t
    utils.repeat_to_batch_size = repeat_to_batch_size
    samplers = types.ModuleType("comfy.samplers")
    samplers.KSAMPLER = type("KSAMPLER", (), {})
    samplers.KSampler = type("KSampler", (), {"SCHEDULERS": ["karras"]})
    mb = types.ModuleType("comfy.model_base")
    mb.ModelType = types.SimpleNamespace(FLUX="FLUX", FLOW="FLOW")
    mb.WAN22 = type("WAN22", (), {})
    ver = types.ModuleType("comfyui_version")
    ver.__version__ = version
    comfy_mod.utils, comfy_mod.samplers, comfy_mod.model_base = utils, samplers, mb
    for name, mod in (("comfy", comfy_mod), ("comfy.utils", utils), ("comfy.samplers", samplers), ("comfy.model_base", mb),
                      ("nodes", types.ModuleType("nodes")), ("latent_preview", types.ModuleType("latent_preview")), ("comfyui_version", ver)):
        sys.modules[name] = mod
    sys.modules.pop("src.LanPaint.nodes", None)
    return importlib.import_module("src.LanPaint.nodes")


def record_calls(Ref, out_path):
    rng = np.random.default_rng(20261016)
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a))      # noqa: E731
    rec = {"n_calls": np.int64(N_CALLS)}
    for i in range(N_CALLS):
        case = {"shape": list(SHAPES[int(rng.integers(len(SHAPES)))]), "flow": bool(rng.integers(2)), "n_steps": int(rng.integers(0, 5)),
                "mask_kind": MASK_KINDS[int(rng.integers(len(MASK_KINDS)))], "form": FORMS[int(rng.integers(len(FORMS)))],
                "lamb": [5.0, 0.5, 12.0][int(rng.integers(3))], "beta": [1.0, 0.5, 2.0][int(rng.integers(3))],
                "step": [0.2, 0.05, 0.6][int(rng.integers(3))], "msf": [0.0, 0.3, 1.0][int(rng.integers(3))],
                "row_sigmas": bool(rng.integers(2)), "stop": STOPS[int(rng.integers(len(STOPS)))], "seed": int(rng.integers(0, 10_001))}
        shape, flow = tuple(case["shape"]), case["flow"]
        sigma, x, y, noise, mask = call_inputs(shape, flow, case["mask_kind"], case["row_sigmas"], case["seed"])
        times = tuple(np.asarray(t, dtype=np.float32) for t in gc.times_from_sigma(sigma, flow))
        mo = None
        if case["stop"] is not None:
            mo = {"lanpaint_semantic_stop": {"threshold": case["stop"][0], "patience": case["stop"][1]}, "lanpaint_semantic_trace": []}
        draws, orig = [], torch.randn_like

        def randn_recorded(t, *a, **k):
            d = orig(t, *a, **k)
            draws.append(d.numpy().copy())
            return d
        model = gc.FormModel(flow, case["form"])
        ref = Ref(model, 5, 15.0, case["lamb"], case["beta"], case["step"], IS_FLUX=False, IS_FLOW=flow, MinStepFrac=case["msf"])
        xr = tt(x.copy())
        torch.manual_seed(case["seed"])
        torch.randn_like = randn_recorded
        try:
            out_r = ref(xr, tt(y), tt(noise), tt(sigma), tt(mask), tuple(tt(t) for t in times), mo, 0, n_steps=case["n_steps"])
        finally:
            torch.randn_like = orig
        case.update(n_draws=len(draws), model_calls=model.calls, trace=None if mo is None else mo["lanpaint_semantic_trace"])
        p = f"c{i}_"
        rec[p + "case"] = np.array(json.dumps(case))
        rec.update({p + "sigma": sigma, p + "x": x, p + "y": y, p + "noise": noise, p + "mask": mask,
                    p + "x_out": xr.numpy(), p + "out": out_r.numpy()})
        for k, d in enumerate(draws):
            rec[f"{p}xi_{k}"] = d
    np.savez_compressed(out_path, **rec)


def record_reshape_mask(ref_root, out_path):
    rec = {}
    saved = {k: sys.modules.get(k) for k in ("comfy", "comfy.utils", "comfy.samplers", "comfy.model_base", "nodes", "latent_preview",
                                             "comfyui_version", "src.LanPaint.nodes")}
    try:
        for version in ("0.6.0", "0.5.0"):
            ref = _reference_nodes(ref_root, version)
            inputs, outputs = [], []
            for m, out_shape, video in gc.random_masks(version):
                inputs.append(gc.array_digest(m))
                try:
                    outputs.append(gc.array_digest(ref.reshape_mask(torch.from_numpy(m), out_shape, video_inpainting=video).numpy()))
                except Exception:
                    outputs.append("")                 # a layout the reference itself rejects
            rec[f"v{version}_input_digests"] = np.array(inputs)
            rec[f"v{version}_output_digests"] = np.array(outputs)
            rec[f"v{version}_effective_steps"] = np.array([ref.min_step_frac_effective_steps(n, f, mf) for n, f, mf in gc.effective_steps_grid()], np.int64)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    np.savez_compressed(out_path, **rec)


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "src", "LanPaint")):
        raise SystemExit("usage: make_reference_calls.py PATH_TO_REFERENCE  (the directory holding src/LanPaint)")
    ref_root = os.path.abspath(sys.argv[1])
    sys.path.insert(0, ref_root)
    sys.dont_write_bytecode = True
    warnings.filterwarnings("ignore")
    Ref = importlib.import_module("src.LanPaint.lanpaint").LanPaint
    record_calls(Ref, os.path.join(HERE, "ref_random_calls.npz"))
    record_reshape_mask(ref_root, os.path.join(HERE, "ref_reshape_mask.npz"))
    for f in ("ref_random_calls.npz", "ref_reshape_mask.npz"):
        print(f, os.path.getsize(os.path.join(HERE, f)), "bytes")


if __name__ == "__main__":
    main()
