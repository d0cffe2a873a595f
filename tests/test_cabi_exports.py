"""The C-ABI library builds for gfx950, loads without a GPU and exports every symbol
include/lanpaint_hip.h declares (no compute calls here)."""
import ctypes
import os
import re

from lanpaint_amd import _cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lanpaint_hip.h")


def _declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(lp_[a-z_0-9]+)\s*\(", src)))


def test_header_functions_are_exported_and_bound(hip_lib):
    names = _declared_functions()
    assert {"lp_coeffs", "lp_step", "lp_finalize", "lp_philox_normal", "lp_boundary_ring", "lp_wmse_pair",
            "lp_reshape_mask", "lp_strerror", "lp_abi_version"} <= set(names)
    for n in names:
        assert hasattr(hip_lib, n), f"{n} declared in the header but not exported"
        assert n in _cabi.EXPORTS, f"{n} has no ctypes binding"


def test_the_c_abi_is_the_only_dynamic_surface(hip_lib):
    """`nm -D --defined-only` of the product library lists the entry points of include/lanpaint_hip.h and
    nothing else -- no lp::*_dispatch, no kernel handles, no __device_stub__ (built with -fvisibility=hidden, every entry
    point LP_API, the rest made local by csrc/exports.map)."""
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", _cabi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip())
    assert syms == _declared_functions(), sorted(set(syms) ^ set(_declared_functions()))
    assert all(s.startswith("lp_") for s in syms) and len(syms) == len(_cabi.EXPORTS)
    hdr = open(HEADER).read()
    for n in syms:                                    # every declaration carries the visibility attribute
        assert re.search(r"LP_API\s+[a-z_0-9 \*]+\b%s\s*\(" % n, hdr), n


# What cabi.hip keeps: the version and error text, the sigma-call family whose launches its own host logic also makes, and the
# entries that block the host or drive graph handles.  Every other entry is defined next to its kernels and begins with its
# argument checks.
_HOST_LOGIC_ENTRIES = {
    "lp_abi_version", "lp_strerror",
    "lp_step", "lp_step_timed", "lp_step_timed_burst", "lp_timer_create", "lp_timer_destroy", "lp_timer_elapsed_ns",
    "lp_coeffs", "lp_finalize", "lp_sigma_times", "lp_sigma_times_mailbox",
    "lp_replay_call", "lp_replay_burst", "lp_graph_bind_replace", "lp_graph_clone_tail", "lp_graph_clone_sigma_root",
    "lp_graph_release", "lp_node_call", "lp_effective_inner_steps"}


def test_every_launching_entry_refuses_null_arguments_before_touching_the_device(hip_lib):
    """Each entry that lives beside its kernels, called with NULL for every pointer and 0 for every number, returns
    LP_E_INVALID -- here, without a GPU, so no HIP call was made on the way.  The excluded names are spelled out and must
    make up EXPORTS together with the called ones: a new entry cannot be left out of both."""
    assert len(_HOST_LOGIC_ENTRIES) == 20 and _HOST_LOGIC_ENTRIES <= set(_cabi.EXPORTS)
    called = {}
    for name, (_res, argtypes) in _cabi.EXPORTS.items():
        if name in _HOST_LOGIC_ENTRIES:
            continue
        args = [None if issubclass(t, (ctypes._Pointer, ctypes.c_void_p, ctypes.c_char_p)) else 0 for t in argtypes]
        called[name] = getattr(hip_lib, name)(*args)
    assert _HOST_LOGIC_ENTRIES | set(called) == set(_cabi.EXPORTS) and len(called) == 65
    wrong = {n: rc for n, rc in called.items() if rc != _cabi.LP_E_INVALID}
    assert not wrong, wrong


def _without_comments(src):
    src = re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), src, flags=re.S)
    return re.sub(r"//[^\n]*", "", src)


def _column0_functions(src):
    """(name, is_definition) of every function declared or defined from column 0: a return type, a name, a parenthesised
    parameter list, then `{` (a definition) or `;` (a prototype).  Macros, static_asserts and variable initialisers have no
    `type name(` shape; calls and nested declarations are indented."""
    out = []
    for m in re.finditer(r'^(?:extern "C" )?(?:template\s*<[^\n]*>\s*)?[A-Za-z_][\w:<>,\*& ]*?[\s\*&]([A-Za-z_]\w*)\s*\(', src, flags=re.M):
        if m.group(1) in ("__attribute__", "__launch_bounds__", "alignas"):
            continue
        depth, i = 1, m.end()
        while depth and i < len(src):
            depth += {"(": 1, ")": -1}.get(src[i], 0)
            i += 1
        rest = src[i:].lstrip()
        while rest.startswith(("const", "noexcept")):
            rest = rest.split(None, 1)[1] if " " in rest else ""
        if rest[:1] in "{;":
            out.append((m.group(1), rest[0] == "{"))
    return out


def test_each_entry_is_defined_once_and_no_source_declares_anothers_function():
    """Every function of include/lanpaint_hip.h has exactly one definition among build.SOURCES, in the one file that holds its
    kernels or in cabi.hip; and no .hip file holds a prototype -- a function another .hip defines is declared in lp_common.h
    or in the public header, where the compiler holds the definition against it."""
    from lanpaint_amd import build
    defined, prototypes = {}, []
    for f in build.SOURCES:
        funcs = _column0_functions(_without_comments(open(os.path.join(build.CSRC, f)).read()))
        assert funcs, f
        for name, is_def in funcs:
            if not is_def:
                prototypes.append((f, name))
            elif name.startswith("lp_") and not name.endswith("_kernel"):
                defined.setdefault(name, []).append(f)
    assert not prototypes, prototypes
    declared = _declared_functions()
    assert len(declared) == len(_cabi.EXPORTS)
    assert {n: defined.get(n, []) for n in declared if len(defined.get(n, [])) != 1} == {}
    assert sorted(defined) == declared, sorted(set(defined) ^ set(declared))


def test_graph_utilities_reject_bad_arguments_without_touching_the_device(hip_lib):
    """lp_replay_burst / lp_graph_clone_sigma_root / lp_graph_bind_replace validate before any HIP call: usable error codes on a
    box without a GPU."""
    import ctypes as C
    d = _cabi.LpStepDesc()
    one = (C.c_void_p * 1)(None)
    assert hip_lib.lp_replay_burst(None, 1, None, None, 1, None) == _cabi.LP_E_INVALID
    assert hip_lib.lp_replay_burst(one, 0, None, None, 1, None) == _cabi.LP_E_INVALID
    assert hip_lib.lp_replay_burst(one, 1, None, None, 0, None) == _cabi.LP_E_INVALID
    g, e, b = C.c_void_p(), C.c_void_p(), _cabi.LpGraphBinding()
    assert hip_lib.lp_graph_clone_sigma_root(None, C.byref(d), C.byref(g), C.byref(e), C.byref(b)) == _cabi.LP_E_INVALID
    d.phases = _cabi.LP_PH_REPLACE | _cabi.LP_PH_EMIT | _cabi.LP_PH_COEFFS          # without LP_PH_SIGMA: not the launch this entry is for
    assert hip_lib.lp_graph_clone_sigma_root(C.c_void_p(1), C.byref(d), C.byref(g), C.byref(e), C.byref(b)) == _cabi.LP_E_INVALID
    assert hip_lib.lp_graph_bind_replace(None, C.byref(d), C.byref(b)) == _cabi.LP_E_INVALID
    assert g.value is None and e.value is None


def _replace_desc(rows=2, el_per_row=1024):
    """A replace launch with the folded coefficient table (the engine's captured node 0) on stand-in device addresses: every
    check plan_step makes passes, and nothing here dereferences them."""
    d = _cabi.LpStepDesc()
    d.n_el, d.rows, d.el_per_row = rows * el_per_row, rows, el_per_row
    d.phases = _cabi.LP_PH_REPLACE | _cabi.LP_PH_EMIT | _cabi.LP_PH_COEFFS
    d.flags = _cabi.LP_FL_MASK_BITS
    d.replace_kind, d.rng_kind = _cabi.LP_REPLACE_VE, _cabi.LP_RNG_PHILOX
    base = 1 << 32
    for k, f in enumerate(("mask", "x_t", "x", "noise", "y", "x_in", "coef_out", "t_abt", "t_ve", "t_rsig")):
        setattr(d, f, base + (k << 20))
    return d


def test_replace_rewrite_refuses_a_binding_of_another_kernel(hip_lib):
    """lp_replay_call with a binding: the rewrite of node 0 is refused unless the replace descriptor dispatches to exactly the
    bound kernel, grid and block -- before any HIP call, and whatever the binding's reserved word holds (a hand-filled binding
    with 0 there used to skip the check)."""
    import ctypes as C
    d = _replace_desc()
    for reserved in (0, 0x1234567):
        b = _cabi.LpGraphBinding()
        b.node, b.func, b.reserved0 = 0x1000, 0xBAD0, reserved
        b.grid[0], b.grid[1], b.grid[2] = 8, 2, 1
        b.block[0], b.block[1], b.block[2] = 256, 1, 1
        call = _cabi.LpCallDesc()
        call.replace, call.graph_exec, call.replace_binding = C.pointer(d), 0x2000, C.pointer(b)
        assert hip_lib.lp_replay_call(C.byref(call), None) == _cabi.LP_E_INVALID


def test_clone_sigma_root_returns_the_dispatch_refusal_before_touching_the_graph(hip_lib):
    import ctypes as C
    g, e, b = C.c_void_p(), C.c_void_p(), _cabi.LpGraphBinding()
    d = _replace_desc(rows=70000, el_per_row=1)          # more rows than a grid holds: lp_step says LP_E_UNSUPPORTED
    d.phases |= _cabi.LP_PH_SIGMA
    d.sg_sigma, d.sg_schedule, d.sg_schedule_len, d.sg_scalars_out = 0x3000, 0x4000, 8, 0x5000
    assert hip_lib.lp_graph_clone_sigma_root(C.c_void_p(1), C.byref(d), C.byref(g), C.byref(e), C.byref(b)) == \
        _cabi.LP_E_UNSUPPORTED
    d = _replace_desc()
    d.phases |= _cabi.LP_PH_SIGMA
    d.sg_sigma, d.sg_schedule, d.sg_schedule_len, d.sg_scalars_out = 0x3000, 0x4000, 0, 0x5000   # an empty schedule
    assert hip_lib.lp_graph_clone_sigma_root(C.c_void_p(1), C.byref(d), C.byref(g), C.byref(e), C.byref(b)) == \
        _cabi.LP_E_INVALID
    assert g.value is None and e.value is None


def test_abi_version_and_strerror(hip_lib):
    assert hip_lib.lp_abi_version() == _cabi.ABI_VERSION
    assert hip_lib.lp_strerror(0) == b"ok"
    for code in (-1, -2, -3, -4, -99):
        assert len(hip_lib.lp_strerror(code)) > 0


def test_engine_refuses_cpu_tensors(hip_lib):
    import pytest
    import torch
    from lanpaint_amd import LanPaint
    from tests.stubs import LinearTupleModel
    eng = LanPaint(LinearTupleModel(), 5, 15.0, 5.0, 1.0, 0.2)
    x = torch.zeros(1, 4, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        eng(x, x, x + 1, torch.tensor([1.0]), x, (torch.tensor([1.0]),) * 3, None, 0)


def test_missing_library_fails_loudly(tmp_path):
    import pytest
    with pytest.raises(ImportError, match="no CPU / PyTorch fallback"):
        _cabi.load(str(tmp_path / "nope.so"))


def test_profiling_variant_builds_and_keeps_the_abi(tmp_path):
    """The -DLP_SHADER_CLOCK build (scripts/shader_clock.py: shader-clock stamps inside the step kernels) compiles for
    gfx950 and is the same library from the outside: same exports, same ABI version.  (Built into build/, never the
    library the package loads by default.)"""
    from lanpaint_amd import build as lpbuild
    out = lpbuild.build(shader_clock=True, verbose=False)
    assert os.path.exists(out) and os.path.abspath(out) != os.path.abspath(_cabi.LIB_PATH)
    lib = _cabi.load(out)
    assert lib.lp_abi_version() == _cabi.ABI_VERSION
    for n in _declared_functions():
        assert hasattr(lib, n)


def test_every_step_kernel_instantiation_is_launched_by_a_gpu_test(hip_lib):
    """lp_step_kernel is one template with seven parameters; the library must hold exactly the instantiations the committed
    coverage file lists, and the GPU suite must have launched every one of them (profiles/r*_instantiation_coverage.json,
    written by scripts/instantiation_coverage.py from a run of the suite against the coverage build).  Adding an
    instantiation without a test that reaches it -- or leaving one behind that nothing launches -- fails here."""
    import glob
    import json
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import instantiation_coverage as ic
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_instantiation_coverage.json")))
    assert files, "no committed instantiation coverage (scripts/instantiation_coverage.py)"
    cov = json.load(open(files[-1]))
    # the DEVICE side is the truth: a kernel can sit in the code object without a host launch stub (round 3 shipped eight)
    have = ic.device_instantiations(_cabi.LIB_PATH)
    stubs = ic.product_instantiations(_cabi.LIB_PATH)
    assert have == stubs, f"device code vs host stubs: device only {sorted(have - stubs)}, host only {sorted(stubs - have)}"
    listed = {i["args"] for i in cov["instantiations"]}
    assert have == listed, f"library vs coverage file: only in library {sorted(have - listed)}, only in file {sorted(listed - have)}"
    assert cov["never_launched"] == [], cov["never_launched"]
    assert set(cov["launched_by_gpu_tests"]) == have
    assert len(have) <= 100, "the instantiation set grew past what round 3 pruned it to; prune or justify"


def test_product_library_reads_nothing_from_the_environment(hip_lib):
    """The header promises a library without global state: no getenv / setenv / secure_getenv among the symbols the
    product .so imports (round 3 read LANPAINT_AMD_TUNE_* into a process-wide static; the switches now travel in
    lp_step_desc.tune), and no LANPAINT_* variable name among its strings."""
    import subprocess
    undefined = subprocess.run(["nm", "-D", "--undefined-only", _cabi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for sym in ("getenv", "secure_getenv", "setenv", "putenv"):
        assert not any(ln.split()[-1].split("@")[0] == sym for ln in undefined.splitlines() if ln.strip()), sym
    blob = open(_cabi.LIB_PATH, "rb").read()
    assert b"LANPAINT_AMD_" not in blob and b"LANPAINT_" not in blob


def test_device_code_holds_only_the_kernels_the_sources_name(hip_lib):
    """Every kernel in the gfx950 code objects is one of ours (lp::...), and the count of step-kernel instantiations on the
    device equals the count of host launch stubs."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import instantiation_coverage as ic
    kernels = ic.device_kernels(_cabi.LIB_PATH)
    assert kernels and all(k.startswith("_ZN2lp") for k in kernels), sorted(k for k in kernels if not k.startswith("_ZN2lp"))[:5]
    assert len(ic.device_instantiations(_cabi.LIB_PATH)) == len(ic.product_instantiations(_cabi.LIB_PATH))


def test_no_kernel_uses_scratch_memory_and_streaming_kernels_fit_eight_waves(hip_lib):
    """Read from the AMDGPU metadata notes of the library that ships (what `hipcc -S` prints as ScratchSize / NumVgprs):
    * no kernel has a private (scratch) segment, spills a VGPR or uses a dynamic stack -- round 4 found first-iteration
      kernels 24-42 % slower than round 3's because of scratch the compiler had introduced (a lambda left as a call, a dropped
      `#pragma unroll`, a load through a pointer selected between a table and a struct field);
    * every phase-specialised 16-bytes-per-lane kernel stays at 8 waves per SIMD: the video latent of BASELINE configs[4] is
      exactly 2048 blocks = 8 per CU, one wave less per SIMD runs it in two rounds (<= 64 VGPRs, <= 100 SGPRs on gfx950)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import instantiation_coverage as ic
    res = ic.kernel_resources(_cabi.LIB_PATH)
    assert len(res) >= len(ic.device_kernels(_cabi.LIB_PATH)) > 80
    for name, k in res.items():
        assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0 and not k[".uses_dynamic_stack"], (name, k)
        assert k[".wavefront_size"] == 64
    # the one exception (both head widths): fp32-mask (soft-mask) first iteration with torch's noise stream in its NON-strided form
    # at 16 bytes per lane -- batches of medium latents whose rows are shorter than half an ATen round -- sits at 102-104 SGPRs =
    # 7 waves (round 5: the replayed graph's generator state is read ahead of the kernel's first store, two more live scalars)
    allowed = {(4, 0, 26, 2, 1, 0, 0), (4, 0, 26, 4, 1, 0, 0)}
    short = []
    for name, k in res.items():
        a = ic.step_kernel_args(name)
        if a and a[0] == 4 and a[2] != 0 and a not in allowed and (k[".vgpr_count"] > 64 or k[".sgpr_count"] > 100):
            short.append((a, k[".vgpr_count"], k[".sgpr_count"]))
    assert not short, short


def test_every_included_file_is_a_build_dependency():
    """Every file a csrc/*.hip or csrc/*.h names in a quoted #include is a source or a header `build.needs_build` looks at: an
    edit to a shared header that is not in `build.HEADERS` would leave a stale library in place."""
    from lanpaint_amd import build
    known = {os.path.basename(p) for p in build.HEADERS} | set(build.SOURCES)
    files = sorted(f for f in os.listdir(build.CSRC) if f.endswith((".hip", ".h")))
    assert "motion_tile.h" in files and set(build.SOURCES) <= set(files)
    included = {}
    for f in files:
        for name in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(os.path.join(build.CSRC, f)).read(), flags=re.M):
            included.setdefault(os.path.basename(name), f)
    assert {"lp_common.h", "motion_tile.h", "mask_tile.h", "resample_tile.h", "lanpaint_hip.h"} <= set(included)
    missing = {name: f for name, f in included.items() if name not in known}
    assert not missing, missing
    assert all(os.path.exists(p) for p in build.HEADERS)
