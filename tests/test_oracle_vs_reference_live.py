"""Differential tests of the oracle against the UNMODIFIED reference, on answers the reference gave and the repository stores
(tests/golden/ref_random_calls.npz, ref_reshape_mask.npz; tests/golden/make_reference_calls.py records them from a reference
tree).  80 engine calls drawn at random over what the fixtures of test_oracle_golden.py do not enumerate: shapes (4-D / 5-D,
odd sizes, batch rows on their own sigmas), VE and flow, hard / soft / all-known / all-inpaint masks, inner-step counts 0..4,
Lambda / Beta / StepSize / MinStepFrac, every model-output form, the inner early stop with its trace.  The oracle consumes the
xi stream the reference consumed; outputs must agree to fp32 rounding."""
import json

import numpy as np
import pytest

from tests import golden_cases as gc
from tests.helpers import load_golden


def test_oracle_equals_the_reference_on_random_calls():
    from oracle.lanpaint_oracle import OracleLanPaint, times_from_sigma
    g = load_golden("ref_random_calls")
    n_calls = int(g["n_calls"])
    assert n_calls >= 80
    with_stop = 0
    for i in range(n_calls):
        p = f"c{i}_"
        case = json.loads(str(g[p + "case"]))
        flow, stop = case["flow"], case["stop"]
        sigma, x, y, noise, mask = (g[p + k] for k in ("sigma", "x", "y", "noise", "mask"))
        times = tuple(np.asarray(t, dtype=np.float32) for t in times_from_sigma(sigma, flow))
        mo = None
        if stop is not None:
            mo = {"lanpaint_semantic_stop": {"threshold": stop[0], "patience": stop[1]}, "lanpaint_semantic_trace": []}
            with_stop += 1
        it = iter([g[f"{p}xi_{k}"] for k in range(case["n_draws"])])
        o_model = gc.FormModel(flow, case["form"])
        o = OracleLanPaint(o_model, 5, 15.0, case["lamb"], case["beta"], case["step"], is_flow=flow, min_step_frac=case["msf"],
                           randn=lambda like: next(it))
        xo = x.copy()
        out_o = o(xo, y, noise, sigma, mask, times, mo, 0, n_steps=case["n_steps"])
        assert sum(1 for _ in it) == 0 and o_model.calls == case["model_calls"], (i, case)
        xr, out_r = g[p + "x_out"], g[p + "out"]
        np.testing.assert_allclose(xo, xr, atol=2e-5 * max(1.0, float(np.abs(xr).max())), rtol=0, err_msg=str((i, case)))
        np.testing.assert_allclose(np.asarray(out_o), out_r, atol=2e-5 * max(1.0, float(np.abs(out_r).max())), rtol=0, err_msg=str((i, case)))
        if mo is not None:
            tr_o, tr_r = mo["lanpaint_semantic_trace"], case["trace"]
            assert len(tr_o) == len(tr_r), (i, case)
            for a, c in zip(tr_o, tr_r):
                assert (a["inner_step"], a["patience_counter"], a["stopped"], a["patience_eff"]) == (c["inner_step"], c["patience_counter"], c["stopped"], c["patience_eff"])
                assert sorted(a) == sorted(c)
                for key in ("dist", "dist_inpaint", "dist_ring", "dist_drift", "threshold_eff", "abt"):
                    assert (a[key] is None) == (c[key] is None), key
                    if a[key] is not None:
                        assert a[key] == pytest.approx(c[key], rel=5e-4, abs=1e-9), key
    assert with_stop >= 20


@pytest.mark.parametrize("version", ["0.6.0", "0.5.0"])
def test_oracle_reshape_mask_equals_the_reference_on_random_masks(version):
    """reshape_mask (nodes.py:59-133) on the mask layouts ComfyUI produces -- [H, W], [B, H, W], [F, H, W] / [F, 1, H, W] video
    masks, the audio forms [F] and [1, 1, F, 1] -- to random latent shapes, both sides of the 0.6.0 gate: BIT-equal (the oracle
    carries the CPU index rules of the torch kernel the reference's F.interpolate runs on a host mask).  The fixture holds
    SHA-256 digests of the reference's outputs ("" where the reference rejects the layout)."""
    from oracle import lanpaint_oracle as orc
    g = load_golden("ref_reshape_mask")
    want_in, want_out = g[f"v{version}_input_digests"], g[f"v{version}_output_digests"]
    new = version == "0.6.0"
    checked = 0
    for k, (m, out_shape, video) in enumerate(gc.random_masks(version)):
        assert gc.array_digest(m) == want_in[k], f"draw {k}: the mask differs from the one the reference was given"
        if not want_out[k]:
            continue                                       # (a layout the reference itself rejects: nothing to mirror)
        got = orc.reshape_mask(m, out_shape, video_inpainting=video, comfy_060_or_newer=new, mask_on="cpu")
        assert gc.array_digest(got) == want_out[k], (k, m.shape, out_shape, video, got.shape)
        checked += 1
    assert k == len(want_in) - 1 and checked >= 250
    # the inner-step rule (nodes.py:134-144) on a dense grid, banker's rounding included
    want = g[f"v{version}_effective_steps"]
    got = [orc.min_step_frac_effective_steps(n, frac, mf) for n, frac, mf in gc.effective_steps_grid()]
    assert len(got) == len(want) and all(a == int(b) for a, b in zip(got, want))
