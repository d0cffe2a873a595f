"""The image-size torch-stream think kernels (one element per lane, phase-specialised, no early stop) at the smallest
shapes at which they can go wrong.

These kernels read the generator state of a replayed graph through a scalar load, take every descriptor field behind one
wait and assume one ATen thread per element (n_el <= rng_bg).  Per case, three sigma calls under one `torch.manual_seed`:

* the engine with `graph=True` (state through the device words) against the same engine with `graph=False` (no state
  pointer, the state by value): `out` and the in-place `x` bitwise equal, the device generator in the same state;
* both against the op-for-op port on the device drawing `torch.randn_like` itself (tests/test_gpu_port_on_device.py, its
  tolerance): a wrong draw or a wrong element -> thread mapping is an O(1) error.

Shapes: 1x4x9x7 (252 elements: bg = 256 != n_el, one partial block), 1x4x17x16 (1 088: several blocks, the last partial),
2x4x16x16 with a sigma per row (row index into the coefficient table, two grid rows).  n_steps 2 (first + last launch) and 3
(first, steady, last); fp32 and bf16 heads; bit-packed hard mask (MODE_HARD) and fp32 soft mask (MODE_ROW); VE and flow.
Routing: a one-element-per-lane torch descriptor past ATen's grid (n_el > rng_bg) plans to the run-time-phase kernel and
draws what lp_torch_normal draws."""
import ctypes
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.stubs import FlowSampling, VESampling      # noqa: E402
from tests.port_checks import PortOnDevice, _compare      # noqa: E402

SHAPES = {"252_one_partial_block": ((1, 4, 9, 7), (1.0,)),
          "1088_partial_last_block": ((1, 4, 17, 16), (1.0,)),
          "two_rows_own_sigma": ((2, 4, 16, 16), (1.0, 0.8))}
SIGMAS = {False: (1.4, 0.9, 0.5), True: (0.8, 0.55, 0.3)}          # three calls, VE / flow


class Heads:
    """fp32 backbone: x -> (0.9 x, 0.8 x).  bf16 backbone: two fixed bf16 tensors, whatever x is -- rounding a function of x to
    bf16 turns the last-bit fp32 differences the port's tolerance allows into whole bf16 steps (4e-3 relative: measured 1.9e-3
    absolute with x -> bf16(0.9 x) under the VE schedule), which says nothing about the kernels; fixed heads keep every
    element's pair of head values distinct (a wrong element mapping or decode still is an O(1) error) and the comparison at the
    fp32 tolerance.  `upcast`: the same VALUES handed on as fp32 (the port's eager ops would otherwise round their own
    intermediates to bf16, which neither the reference on fp32 heads nor the kernel does)."""

    def __init__(self, flow, dtype, upcast, shape):
        import torch
        self.inner_model = self
        self.model_sampling = FlowSampling() if flow else VESampling()
        self.dtype, self.upcast = dtype, upcast
        g = torch.Generator(device="cuda").manual_seed(23)
        self.fixed = tuple(torch.randn(shape, device="cuda", generator=g).to(dtype) for _ in range(2))

    def __call__(self, x, t, model_options=None, seed=None):
        import torch
        if self.dtype == torch.float32:
            return 0.9 * x, 0.8 * x
        a, b = self.fixed
        return (a.float(), b.float()) if self.upcast else (a.clone(), b.clone())


def _job(shape, ramp, flow, soft):
    import torch
    import bench
    from lanpaint_amd import pack_mask
    g = torch.Generator(device="cuda").manual_seed(17)
    y = torch.randn(shape, device="cuda", generator=g)
    noise = torch.randn(shape, device="cuda", generator=g)
    u = torch.rand(shape, device="cuda", generator=g)
    mask = u if soft else (u < 0.5).float()
    r = torch.tensor(ramp, device="cuda", dtype=torch.float32)
    sig_list = [r * s for s in SIGMAS[flow]]
    rb = (sig_list[0]).reshape((-1,) + (1,) * (len(shape) - 1))
    x0 = (rb * noise + (1 - rb) * y) if flow else (y + noise * rb)
    return dict(x0=x0, y=y, noise=noise, mask=mask, mask_product=mask if soft else pack_mask(mask.clone()), sig_list=sig_list,
                times_list=[bench.times_from_sigma(s, flow) for s in sig_list], ratios=bench.euler_ratios(sig_list, len(shape)))


def _walk(engine, job, mask, n_steps, seed):
    import torch
    torch.manual_seed(seed)
    x = job["x0"].clone()
    outs, xs = [], []
    with torch.no_grad():
        for i, (s, t) in enumerate(zip(job["sig_list"], job["times_list"])):
            den = engine(x, job["y"], job["noise"], s, mask, t, None, 0, n_steps=n_steps)
            outs.append(den.clone())
            xs.append(x.clone())
            if i + 1 < len(job["sig_list"]):
                x = torch.lerp(den, x, job["ratios"][i])
    torch.cuda.synchronize()
    return outs, xs, torch.cuda.get_rng_state(0).clone()


def _product(job, flow, dtype, n_steps, seed, graph):
    import bench
    from lanpaint_amd import LanPaint
    h = bench.HYPER
    eng = LanPaint(Heads(flow, dtype, False, tuple(job["x0"].shape)), n_steps, h["Friction"], h["Lambda"], h["Beta"], h["StepSize"], False, flow, graph=graph)
    assert eng.rng == "torch"
    res = _walk(eng, job, job["mask_product"], n_steps, seed)
    assert bool(eng._graphs) == bool(graph)
    return eng, res


@pytest.mark.parametrize("flow", [False, True], ids=["ve", "flow"])
@pytest.mark.parametrize("soft", [False, True], ids=["hard_bits", "soft_f32"])
@pytest.mark.parametrize("heads", ["f32", "bf16"])
@pytest.mark.parametrize("n_steps", [2, 3])
@pytest.mark.parametrize("shape_id", list(SHAPES))
def test_replayed_and_eager_launches_agree_bitwise_and_match_the_port(shape_id, n_steps, heads, soft, flow):
    import torch
    import bench
    from lanpaint_amd import _cabi
    shape, ramp = SHAPES[shape_id]
    dtype = torch.bfloat16 if heads == "bf16" else torch.float32
    job = _job(shape, ramp, flow, soft)
    seed = 4242
    eng_g, (out_g, x_g, st_g) = _product(job, flow, dtype, n_steps, seed, True)
    eng_e, (out_e, x_e, st_e) = _product(job, flow, dtype, n_steps, seed, False)
    # the launches under test: phase-specialised (never the run-time-phase kernel), the mask form asked for
    fl = eng_g._desc.flags
    assert bool(fl & _cabi.LP_FL_MASK_BITS) == (not soft), "mask format seen by the kernels"
    for i, (a, b, c, d) in enumerate(zip(out_g, out_e, x_g, x_e)):
        assert torch.equal(a, b), f"sigma call {i}: out differs between replayed and eager launches"
        assert torch.equal(c, d), f"sigma call {i}: in-place x differs between replayed and eager launches"
    assert torch.equal(st_g, st_e), "replayed and eager launches leave the device generator in different states"
    h = bench.HYPER
    port = PortOnDevice(Heads(flow, dtype, True, shape), n_steps, h["Friction"], h["Lambda"], h["Beta"], h["StepSize"], False, flow)
    out_p, x_p, st_p = _walk(port, job, job["mask"], n_steps, seed)
    for tag, outs, xs, st in (("replayed", out_g, x_g, st_g), ("eager", out_e, x_e, st_e)):
        for i, (a, b, c, d) in enumerate(zip(outs, out_p, xs, x_p)):
            _compare(a, b, f"{tag}, sigma call {i}: out")
            _compare(c, d, f"{tag}, sigma call {i}: in-place x")
        assert torch.equal(st, st_p), f"{tag}: the product leaves the device generator in another state than the port"


def test_another_seed_fails_the_equality():
    """Teeth: the bitwise comparison is not vacuous."""
    import torch
    shape, ramp = SHAPES["1088_partial_last_block"]
    job = _job(shape, ramp, False, False)
    _, (out_a, x_a, _) = _product(job, False, torch.float32, 3, 1, True)
    _, (out_b, x_b, _) = _product(job, False, torch.float32, 3, 2, False)
    assert not torch.equal(out_a[-1], out_b[-1]) and not torch.equal(x_a[0], x_b[0])
    assert float((out_a[-1] - out_b[-1]).abs().max()) > 1e-2


# ------------------------------------------------------------------ routing: past ATen's grid at one element per lane
@pytest.mark.parametrize("bg", [4096, 1280], ids=["bg_power_of_two", "bg_5_blocks"])
@pytest.mark.parametrize("phase", ["steady", "first", "last"])
@pytest.mark.parametrize("mask_format", ["bits", "f32"])
def test_descriptor_past_atens_grid_draws_what_lp_torch_normal_draws(mask_format, phase, bg):
    """16 384 elements with a hand-made grid of 4 096 / 1 280 ATen threads (n_el > rng_bg), handed to lp_step directly: thread j
    serves elements j, j + bg, ... -- four per Philox block.  The image-size kernels would draw every element from its own
    block; the plan has to send the descriptor to the run-time-phase kernel.  The library exports no plan query, so the
    routing is checked by what it decides: x_t, C and x_in must be BITWISE what the same launch gives when both draws are
    handed in as tensors filled by lp_torch_normal for the same (seed, offset, bg) -- a launch on the image-size kernel
    differs in every element from index bg on."""
    import torch
    import bench
    from lanpaint_amd import _cabi
    lib = _cabi.load()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    S, F, P, E = _cabi.LP_PH_POST_STEADY, _cabi.LP_PH_POST_FIRST, _cabi.LP_PH_PRE_HALF, _cabi.LP_PH_EMIT
    ph = {"steady": S | P | E, "first": F | P | E, "last": S | E}[phase]
    res = []
    for host_noise in (False, True):
        d, keep, n_el = bench.standalone_step(_cabi, "c1_sd15", dev, ph, mask_format=mask_format, rng="torch")
        assert n_el == 16384 and n_el > bg
        d.tune = _cabi.LP_TUNE_VEC1
        d.rng_bg, d.rng_inc = bg, ((n_el - 1) // (bg * 4) + 1) * 4
        d.rng_seed, d.rng_offset = 77, 8
        if host_noise:
            xi = [torch.empty(n_el, device=dev) for _ in range(2)]
            for k, t in enumerate(xi):
                _cabi.check(lib.lp_torch_normal(t.data_ptr(), n_el, 77, 8 + k * d.rng_inc, bg, st), "lp_torch_normal")
            d.xi_post, d.xi_pre = xi[0].data_ptr(), xi[1].data_ptr()
        _cabi.check(lib.lp_step(ctypes.byref(d), st), "lp_step")
        torch.cuda.synchronize()
        bufs = keep[0]
        res.append(tuple(bufs[k].clone() for k in ("x_t", "C", "x_in")))
    for name, a, b in zip(("x_t", "C", "x_in"), *res):
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, b), f"{name}: {int((a != b).sum())} elements differ, first at {int((a != b).flatten().nonzero()[0]) if (a != b).any() else -1}"
