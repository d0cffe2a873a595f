"""The engine port held to the product on the device, and the AV case both of its tests use."""
import numpy as np

from oracle import lanpaint_oracle as orc


def _case(shape, split, seed, soft=False, rows_differ=False):
    rng = np.random.default_rng(seed)
    b = shape[0]
    y = rng.standard_normal(shape, dtype=np.float32)
    noise = rng.standard_normal(shape, dtype=np.float32)
    ai = np.zeros(shape, dtype=np.float32)
    ai[..., split:] = 1.0                                    # the audio part of the flat pack
    mask = (rng.random(shape) > 0.45).astype(np.float32)
    if soft:
        mask = rng.random(shape, dtype=np.float32)
    t_v = np.float32([0.55 + (0.1 * r if rows_differ else 0.0) for r in range(b)])
    t_a = np.float32([0.30 + (0.05 * r if rows_differ else 0.0) for r in range(b)])
    if b > 1:            # (the reference blends `times * (1 - ai)`: per-row times of a batch have to broadcast against the latent)
        t_v, t_a = t_v.reshape((b,) + (1,) * (len(shape) - 1)), t_a.reshape((b,) + (1,) * (len(shape) - 1))
    times_v = orc.times_from_sigma(t_v, True)
    times_a = orc.times_from_sigma(t_a, True)
    corr = ((1.0 - ai) + np.float32(0.7) * ai).astype(np.float32)
    bs = (-1,) + (1,) * (len(shape) - 1)
    x = (t_v.reshape(bs) * noise + (1 - t_v.reshape(bs)) * y).astype(np.float32)
    t_v = np.ascontiguousarray(t_v)
    return dict(x=x, y=y, noise=noise, mask=mask, ai=ai, sigma=t_v, times_v=times_v, times_a=times_a, corr=corr)


REL, MSE = 2e-5, 1e-9


class PortOnDevice:
    """The port behind the reference's constructor / call signature (lanpaint.py:8,44): the replace step goes through the
    model_sampling's own noise_scaling like the reference's does (lanpaint.py:84-92)."""

    def __init__(self, Model, NSteps, Friction, Lambda, Beta, StepSize, IS_FLUX=False, IS_FLOW=False, EarlyStopThreshold=0.0,
                 EarlyStopPatience=1, EarlyStopHook=None, MinStepFrac=0.0):
        from oracle.lanpaint_oracle import OracleLanPaint, TorchBackend
        ms = Model.inner_model.model_sampling
        self.inner_model = Model
        self.port = OracleLanPaint(Model, NSteps, Friction, Lambda, Beta, StepSize, is_flux=IS_FLUX, is_flow=IS_FLOW,
                                   early_stop_threshold=EarlyStopThreshold, early_stop_patience=EarlyStopPatience,
                                   min_step_frac=MinStepFrac, backend=TorchBackend(), noise_scaling=ms.noise_scaling,
                                   noise_scale=float(getattr(ms, "noise_scale", 1.0)))

    def __call__(self, x, latent_image, noise, sigma, latent_mask, current_times, model_options, seed, n_steps=None, **kw):
        return self.port(x, latent_image, noise, sigma, latent_mask, current_times, model_options, seed, n_steps=n_steps, **kw)


def _compare(got, want, what):
    import torch
    g, w = got.double(), want.double()
    assert torch.isfinite(g).all(), f"{what}: non-finite values"
    scale = max(1.0, float(w.abs().max()))
    err = float((g - w).abs().max())
    mse = float(((g - w) ** 2).mean())
    assert err <= REL * scale, f"{what}: max abs err {err:.3e} > {REL * scale:.3e}"
    assert mse <= MSE * scale * scale, f"{what}: MSE {mse:.3e}"
    return err / scale, mse
