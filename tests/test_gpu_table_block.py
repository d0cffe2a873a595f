"""The fused replace launch (LP_PH_REPLACE | LP_PH_EMIT | LP_PH_COEFFS [| LP_PH_SIGMA]) builds the coefficient table, publishes
the generator state and runs the sigma rule on a table block of its own: block (0, row) of a grid one block wider than the
element work.  What that block writes must equal what the separate kernels write, bit for bit, and the graph entry points must
follow the wider grid."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from lanpaint_amd import _cabi
    return _cabi.load()


def _setup(rows, flow, dev, el_per_row=4 * 64 * 64):
    import torch
    from benchkit.workloads import attach_mask_format, times_from_sigma
    from lanpaint_amd import _cabi
    g = torch.Generator(device=dev).manual_seed(rows * 2 + int(flow))
    shape = (rows, el_per_row)
    x, y, noise = (torch.randn(shape, device=dev, generator=g) for _ in range(3))
    mask = attach_mask_format((torch.rand(shape, device=dev, generator=g) < 0.5).float(), "bits")
    sig = torch.linspace(0.3, 0.8, rows, device=dev) if flow else torch.linspace(0.6, 6.0, rows, device=dev)
    ve, abt, ft = times_from_sigma(sig, flow)
    d = _cabi.LpStepDesc()
    d.n_el, d.el_per_row, d.rows = rows * el_per_row, el_per_row, rows
    d.flags = _cabi.LP_FL_MASK_BITS | (_cabi.LP_FL_FLOW if flow else 0)
    d.replace_kind = _cabi.LP_REPLACE_FLOW if flow else _cabi.LP_REPLACE_VE
    d.lambda_, d.one_plus_lambda, d.beta, d.step_size, d.min_step_frac, d.noise_scale = 5.0, 6.0, 1.3, 0.2, 0.1, 1.0
    d.x, d.noise, d.y, d.mask = x.data_ptr(), noise.data_ptr(), y.data_ptr(), mask._lp_bits.data_ptr()
    d.phases = _cabi.LP_PH_REPLACE | _cabi.LP_PH_EMIT | _cabi.LP_PH_COEFFS
    tm = ft if flow else ve
    keep = [x, y, noise, mask, sig, ve, abt, tm]
    return d, keep


def _hyper(d, flow):
    from lanpaint_amd import _cabi
    h = _cabi.LpHyper()
    h.lambda_, h.beta, h.step_size, h.min_step_frac = d.lambda_, d.beta, d.step_size, d.min_step_frac
    h.is_flow, h.one_plus_lambda = int(flow), d.one_plus_lambda
    return h


@pytest.mark.parametrize("fold_sigma", [False, True])
@pytest.mark.parametrize("rows", [1, 4])
@pytest.mark.parametrize("flow", [False, True])
def test_table_block_writes_what_the_separate_kernels_write(lib, flow, rows, fold_sigma):
    import torch
    from lanpaint_amd import _cabi
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    d, keep = _setup(rows, flow, dev)
    x, y, noise, mask, sig, ve, abt, tm = keep
    # the separate kernels: lp_sigma_times_mailbox (times, rule scalars, mailbox), lp_coeffs, the unfused replace launch
    sched = torch.linspace(0.1, 8.0, 17, device=dev) if not flow else torch.linspace(0.05, 0.95, 17, device=dev)
    times_ref = torch.full((3, rows), float("nan"), device=dev)
    scal_ref = torch.full((4,), float("nan"), device=dev)
    seq_ref = torch.zeros(1, dtype=torch.int32, device=dev)
    _cabi.check(lib.lp_sigma_times_mailbox(sig.data_ptr(), rows, sched.data_ptr(), 17, int(flow), times_ref.data_ptr(),
                                           scal_ref.data_ptr(), seq_ref.data_ptr(), 7, st), "lp_sigma_times_mailbox")
    coef_ref = torch.full((rows, _cabi.LP_COEF_STRIDE), float("nan"), device=dev)
    _cabi.check(lib.lp_coeffs(ctypes.byref(_hyper(d, flow)), ve.data_ptr(), 1, abt.data_ptr(), 1, sig.data_ptr(), 1, None, 0,
                              tm.data_ptr(), 1, rows, coef_ref.data_ptr(), st), "lp_coeffs")
    x_t_ref, x_in_ref = torch.empty_like(x), torch.empty_like(x)
    d.phases = _cabi.LP_PH_REPLACE | _cabi.LP_PH_EMIT
    d.coef, d.x_t, d.x_in = coef_ref.data_ptr(), x_t_ref.data_ptr(), x_in_ref.data_ptr()
    _cabi.check(lib.lp_step(ctypes.byref(d), st), "lp_step (unfused)")

    # the fused launch
    coef = torch.full((rows, _cabi.LP_COEF_STRIDE), float("nan"), device=dev)
    x_t, x_in = torch.empty_like(x), torch.empty_like(x)
    rng_out = torch.zeros(2, dtype=torch.int64, device=dev)
    d.phases = _cabi.LP_PH_REPLACE | _cabi.LP_PH_EMIT | _cabi.LP_PH_COEFFS
    d.coef, d.coef_out, d.x_t, d.x_in = None, coef.data_ptr(), x_t.data_ptr(), x_in.data_ptr()
    d.rng_state_out = rng_out.data_ptr()
    d.rng_state_val[0], d.rng_state_val[1] = 0x123456789, 0xABCDEF
    times = torch.full((3, rows), float("nan"), device=dev)
    scal = torch.full((4,), float("nan"), device=dev)
    seq = torch.zeros(1, dtype=torch.int32, device=dev)
    valid = torch.zeros(1, dtype=torch.int64, device=dev)
    if fold_sigma:
        d.phases |= _cabi.LP_PH_SIGMA
        d.sg_sigma, d.sg_schedule, d.sg_schedule_len = sig.data_ptr(), sched.data_ptr(), 17
        d.sg_times_out, d.sg_scalars_out, d.sg_seq_out, d.sg_seq = times.data_ptr(), scal.data_ptr(), seq.data_ptr(), 7
        d.sg_valid_out, d.sg_min_step_frac = valid.data_ptr(), 0.1
        d.sg_n_steps, d.sg_early_stop, d.sg_total_steps, d.sg_guess = 5, 0, 30, 5
    else:
        d.t_ve, d.t_abt, d.t_rsig, d.t_model = ve.data_ptr(), abt.data_ptr(), sig.data_ptr(), tm.data_ptr()
        d.t_ve_stride = d.t_abt_stride = d.t_rsig_stride = d.t_model_stride = 1
    _cabi.check(lib.lp_step(ctypes.byref(d), st), "lp_step (fused)")
    torch.cuda.synchronize()
    # the table's fields lp_coeffs writes (the rest of the stride is padding)
    used = [c for c in range(_cabi.LP_COEF_STRIDE) if c < 32 or c == _cabi.LP_C_TMODEL]
    assert torch.equal(coef[:, used].view(torch.int32), coef_ref[:, used].view(torch.int32))
    assert torch.equal(x_t, x_t_ref) and torch.equal(x_in, x_in_ref)
    assert rng_out.tolist() == [0x123456789, 0xABCDEF]
    if fold_sigma:
        assert torch.equal(times.view(torch.int32), times_ref.view(torch.int32))
        assert torch.equal(scal[:2].view(torch.int32), scal_ref[:2].view(torch.int32))
        assert int(seq.item()) == 7 == int(seq_ref.item())


def test_graph_binding_follows_the_table_block_grid(lib):
    """A captured fused replace launch runs on ceil(groups / 256) + 1 blocks per row; lp_graph_bind_replace binds that
    grid, and a rewrite through a binding that names the grid without the table block is refused."""
    import torch
    from lanpaint_amd import _cabi
    dev = torch.device("cuda", 0)
    rows, epr = 2, 4 * 64 * 64
    d, keep = _setup(rows, False, dev, epr)
    _x, _y, _n, _m, sig, ve, abt, tm = keep
    coef = torch.empty((rows, _cabi.LP_COEF_STRIDE), device=dev)
    x_t, x_in = torch.empty((rows, epr), device=dev), torch.empty((rows, epr), device=dev)
    d.coef_out, d.x_t, d.x_in = coef.data_ptr(), x_t.data_ptr(), x_in.data_ptr()
    d.t_ve, d.t_abt, d.t_rsig, d.t_model = ve.data_ptr(), abt.data_ptr(), sig.data_ptr(), tm.data_ptr()
    d.t_ve_stride = d.t_abt_stride = d.t_rsig_stride = d.t_model_stride = 1
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    try:
        graph = torch.cuda.CUDAGraph(keep_graph=True)
    except TypeError:
        pytest.skip("torch without CUDAGraph(keep_graph=True)")
    with torch.cuda.graph(graph, stream=side):
        _cabi.check(lib.lp_step(ctypes.byref(d), side.cuda_stream), "lp_step")
    torch.cuda.synchronize()
    b = _cabi.LpGraphBinding()
    assert lib.lp_graph_bind_replace(ctypes.c_void_p(int(graph.raw_cuda_graph())), ctypes.byref(d), ctypes.byref(b)) == _cabi.LP_OK
    assert (b.grid[0], b.grid[1], b.grid[2]) == (epr // 256 + 1, rows, 1)
    # (the refusal comes before any HIP call: the executable graph is never touched)
    stale = _cabi.LpGraphBinding()
    ctypes.memmove(ctypes.byref(stale), ctypes.byref(b), ctypes.sizeof(b))
    stale.grid[0] = epr // 256
    call = _cabi.LpCallDesc()
    call.replace, call.graph_exec, call.replace_binding = ctypes.pointer(d), 0x2000, ctypes.pointer(stale)
    assert lib.lp_replay_call(ctypes.byref(call), None) == _cabi.LP_E_INVALID
    torch.cuda.synchronize()
    del graph
