"""lanpaint_amd/_cabi.py is a hand-written mirror of include/lanpaint_hip.h; here the whole of it is held against the header, as
tests/cabi_header.py reads it and as gcc lays it out: every struct, field, prototype and constant, with nothing chosen by hand.
A new descriptor needs no layout test of its own -- only an entry in SIZES if its size is worth a pin.  The names of every module
and the protocol of every node module are checked the same way, found by glob.  No GPU, one gcc run.

The rules, in the order of the tests below: 1 structs both ways, 2 field names, order and types, 3 offsets and sizes (with SIZES
and OFFSETS), 4 prototypes, 5 constants (with PINS and RESTATED), 6 macros with a Python twin (MACROS), 7 the ABI version, 8 the
version script, 9 unbound names, 10 node modules."""
import ctypes as C
import glob
import importlib
import os
import re
import subprocess
import sys

import pytest

from lanpaint_amd import _cabi
from tests import cabi_header
from tests.cabi_header import _call

ROOT = cabi_header.ROOT
HEADER = cabi_header.parse()
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
           "uint8_t": C.c_uint8, "float": C.c_float, "double": C.c_double}
MIRROR = {name: getattr(_cabi, cabi_header.class_name(name), None) for name in HEADER.structs}
CONSTANTS = sorted(n for n, v in vars(_cabi).items() if n.startswith("LP_") and isinstance(v, (int, float)))

# lp_prop_fill_batch takes `const lp_prop_fill_job*` and is bound as c_void_p: its one caller passes the address of a numpy table
UNTYPED_STRUCT_ARGUMENTS = {"lp_prop_fill_batch"}

# ---- the literal pins the per-module layout tests used to carry, one table each ---------------------------------------------------
SIZES = {
    "lp_prop_anchor_desc": 64, "lp_prop_anchor_gated_desc": 80, "lp_prop_match_batch_desc": 40,
    "lp_prop_match_job": 48, "lp_prop_advance_job": 48,
    "lp_prop_visible_job": 40, "lp_prop_visible_batch_desc": 24, "lp_prop_occlude_job": 48, "lp_prop_occlude_batch_desc": 24,
    "lp_prop_merge_visible_desc": 120, "lp_prop_visible_desc": 56, "lp_prop_occlude_desc": 56,
}
OFFSETS = {("lp_prop_match_batch_desc", "reserved0"): 28}
PINS = {
    "LP_COLOR_MIN_COUNT": 64, "LP_COLOR_MAX_MARGIN": 25,
    "LP_GRAIN_BANDS": 8, "LP_GRAIN_MIN_COUNT": 64, "LP_GRAIN_WHITE_VAR": 21845, "LP_GRAIN_MAX_STD": 64, "LP_GRAIN_MAX_MARGIN": 25,
    "LP_GRAIN_TILE_H": 16, "LP_GRAIN_TILE_W": 64, "LP_GRAIN_REGION_ALL": 0, "LP_GRAIN_REGION_OUTSIDE": 1, "LP_GRAIN_REGION_INSIDE": 2,
    "LP_GRAIN_SIZE_AUTO": -1,
    "LP_PROP_BLOCK": 8, "LP_PROP_HALO": 4, "LP_PROP_MIN_PIXELS": 16, "LP_PROP_FILL_ITERS": 3, "LP_PROP_SUBPEL": 16,
    "LP_PROP_MAX_LEVELS": 6, "LP_PROP_MAX_SEARCH": 7, "LP_PROP_MAX_SMOOTH": 64, "LP_PROP_ALIGN": 16, "LP_PROP_MAX_GRID": 2048,
    "LP_PROP_MAX_JOBS": 32, "LP_PROP_MATCH_WARPED_KEY": 1, "LP_PROP_VIS_MAX_BIAS": 32,
    "LP_REFINE_MAX_RADIUS": 64, "LP_TSMOOTH_ROBUST_QUORUM": 2,
    "LP_STAB_MAX_MEDIAN": 3, "LP_STAB_MAX_SMOOTH": 8, "LP_STAB_MAX_GROW": 256, "LP_STAB_MAX_FEATHER": 64,
}
# (restatement module under tests/, its name, what it must equal): the CPU restatements state the header's constants again
RESTATED = [
    ("color_ref", "MIN_COUNT", _cabi.LP_COLOR_MIN_COUNT),
    ("grain_ref", "K", _cabi.LP_GRAIN_BANDS), ("grain_ref", "MIN_COUNT", _cabi.LP_GRAIN_MIN_COUNT),
    ("grain_ref", "WHITE_VAR", _cabi.LP_GRAIN_WHITE_VAR), ("grain_ref", "MAX_STD", _cabi.LP_GRAIN_MAX_STD),
    ("grain_ref", "MAX_MARGIN", _cabi.LP_GRAIN_MAX_MARGIN), ("grain_ref", "ALL", _cabi.LP_GRAIN_REGION_ALL),
    ("grain_ref", "OUTSIDE", _cabi.LP_GRAIN_REGION_OUTSIDE), ("grain_ref", "INSIDE", _cabi.LP_GRAIN_REGION_INSIDE),
    ("grain_ref", "AUTO", _cabi.LP_GRAIN_SIZE_AUTO),
    ("propagate_ref", "BLOCK", 8), ("propagate_ref", "HALO", 4), ("propagate_ref", "MIN_PIXELS", 16), ("propagate_ref", "FILL_ITERS", 3),
    ("propagate_visible_ref", "VIS_MAX_BIAS", _cabi.LP_PROP_VIS_MAX_BIAS),
    ("shots_ref", "MAX_SEARCH", 3), ("shots_ref", "MAX_WINDOW", 16), ("shots_ref", "BINS", 64),
    ("shots_ref", "MAX_LEVEL", _cabi.LP_PROP_MAX_LEVELS - 1),
    ("temporal_fill_checked_ref", "DISPUTED", _cabi.LP_TFILL_DISPUTED), ("temporal_fill_checked_ref", "MAX_BIAS", _cabi.LP_PROP_VIS_MAX_BIAS),
    ("temporal_fill_checked_ref", "MIN_PIXELS", _cabi.LP_PROP_MIN_PIXELS), ("temporal_fill_checked_ref", "BLOCK", _cabi.LP_PROP_BLOCK),
    ("temporal_smooth_robust_ref", "QUORUM", _cabi.LP_TSMOOTH_ROBUST_QUORUM),
]
# (function-like macro of the header, its Python twin in _cabi, the argument values the per-module tests used)
MACROS = [
    ("LP_COLOR_WS_BYTES", _cabi.lp_color_ws_bytes,
     [(1, 1, 1, 1), (2, 17, 33, 3), (7, 32, 128, 4), (3, 33, 129, 5), (81, 576, 1024, 3), (65535, 32768, 32768, 64)]),
    ("LP_COMPONENTS_WS_BYTES", _cabi.lp_components_ws_bytes, [(720, 1280), (32768, 32768)]),
    ("LP_COMPONENTS_FRAMES_WS_BYTES", _cabi.lp_components_frames_ws_bytes, [(1, 1, 1), (81, 720, 1280), (65535, 128, 128), (1, 720, 1280)]),
    ("LP_PROP_MATCH_GATED", _cabi.LP_PROP_MATCH_GATED, [(16,), (1,), (255,)]),
]


@pytest.fixture(scope="module")
def c_values(tmp_path_factory):
    """What gcc makes of the header, from ONE program: "struct.field" -> offsetof, "struct" -> sizeof, "LP_X" -> its value,
    "LP_X(args)" -> its value at the arguments of MACROS."""
    show = lambda key, fmt, expr: 'printf("%s\\t{}\\n", "{}", {});'.format(fmt, key, expr)       # noqa: E731
    prog = ["#include <stdio.h>", "#include <stddef.h>", '#include "lanpaint_hip.h"', "int main(void){"]
    for struct, fields in HEADER.structs.items():
        prog.append(show(struct, "%zu", f"sizeof({struct})"))
        prog += [show(f"{struct}.{f.name}", "%zu", f"offsetof({struct}, {f.name})") for f in fields]
    prog += [show(name, "%.17g", f"(double)({name})") for name in CONSTANTS + ["LP_ABI_VERSION"] if name in HEADER.defines]
    prog += [show(_call(m, a), "%lld", f"(long long){_call(m, a)}") for m, _, cases in MACROS for a in cases]
    prog.append("return 0;}")
    tmp = tmp_path_factory.mktemp("cabi_mirror")
    (tmp / "mirror.c").write_text("\n".join(prog))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp / "mirror.c"), "-o", str(tmp / "mirror")], check=True)
    out = subprocess.run([str(tmp / "mirror")], check=True, capture_output=True, text=True).stdout
    values = {key: float(v) if "." in v or "e" in v else int(v) for key, v in (line.split("\t") for line in out.splitlines())}
    assert len(values) == len(prog) - 5
    return values


def _allowed(base, ptr, typed_structs=False):
    """The ctypes types that may stand for `base` behind `ptr` stars.  A scalar is exactly its ctypes type and a struct by value its
    mirrored class; a pointer is c_void_p or a POINTER to what it names (`const char*` is c_char_p).  `typed_structs`: a pointer
    straight to a struct must be the POINTER to its class."""
    if ptr == 0:
        return {SCALARS[base]} if base in SCALARS else {MIRROR[base]}
    if (base, ptr) == ("char", 1):
        return {C.c_char_p}
    if (base, ptr) == ("void", 1):
        return {C.c_void_p}
    typed = {C.POINTER(t) for t in _allowed(base, ptr - 1)}
    return typed if typed_structs and ptr == 1 and base in MIRROR else typed | {C.c_void_p}


def _fits(ctype, decl, typed_structs=False):
    if decl.length is None:
        return ctype in _allowed(decl.base, decl.ptr, typed_structs)
    return issubclass(ctype, C.Array) and ctype._length_ == decl.length and ctype._type_ in _allowed(decl.base, decl.ptr)


def test_every_struct_of_the_header_has_a_class_and_every_class_a_struct():
    classes = {v.__name__ for v in vars(_cabi).values() if isinstance(v, type) and issubclass(v, C.Structure)}
    assert {cabi_header.class_name(name) for name in HEADER.structs} == classes and len(classes) == len(HEADER.structs) >= 58
    assert cabi_header.class_name("lp_prop_match_job") == "LpPropMatchJob" and cabi_header.field_name("lambda") == "lambda_"


def test_every_field_has_the_headers_name_order_and_type():
    wrong = []
    for struct, fields in HEADER.structs.items():
        mirrored = MIRROR[struct]._fields_
        assert [name for name, _ in mirrored] == [cabi_header.field_name(f.name) for f in fields], struct
        wrong += [(struct, f, ctype) for f, (_, ctype) in zip(fields, mirrored) if not _fits(ctype, f)]
    assert not wrong, wrong


def test_every_offset_and_size_is_what_gcc_lays_out(c_values):
    wrong = {}
    for struct, fields in HEADER.structs.items():
        py = MIRROR[struct]
        got = {struct: C.sizeof(py), **{f"{struct}.{f.name}": getattr(py, cabi_header.field_name(f.name)).offset for f in fields}}
        wrong.update({key: (c_values[key], v) for key, v in got.items() if c_values[key] != v})
    assert not wrong, wrong
    assert {s: c_values[s] for s in SIZES} == SIZES
    assert {k: c_values["%s.%s" % k] for k in OFFSETS} == OFFSETS


def test_every_prototype_has_its_restype_and_argtypes():
    assert set(HEADER.functions) == set(_cabi.EXPORTS) and len(HEADER.functions) >= 85
    wrong, untyped = [], set()
    for name, fn in HEADER.functions.items():
        restype, argtypes = _cabi.EXPORTS[name]
        assert len(argtypes) == len(fn.args), name
        if not _fits(restype, fn.result):
            wrong.append((name, "result", restype))
        for arg, ctype in zip(fn.args, argtypes):
            if _fits(ctype, arg, typed_structs=True):
                continue
            if _fits(ctype, arg):
                untyped.add(name)
            else:
                wrong.append((name, arg, ctype))
    assert not wrong, wrong
    assert untyped == UNTYPED_STRUCT_ARGUMENTS


def test_every_constant_is_the_headers(c_values):
    assert sorted(set(CONSTANTS) - set(HEADER.defines)) == [], "LP_* constants of _cabi the header does not define"
    compared = {name: (getattr(_cabi, name), c_values[name]) for name in CONSTANTS}
    assert {n: v for n, v in compared.items() if v[0] != v[1]} == {}
    assert len(compared) == len([n for n in vars(_cabi) if n.startswith("LP_") and not callable(getattr(_cabi, n))]) >= 130
    assert {n: getattr(_cabi, n) for n in PINS} == PINS
    assert _cabi.LP_PROP_MAX_GRID == -(-_cabi.LP_VMASK_MAX_SIDE // _cabi.LP_PROP_BLOCK)
    # the job table travels by value in the kernel's arguments: 32 x 48 bytes, inside the 4 KB limit
    assert _cabi.LP_PROP_MAX_JOBS * 48 + 64 <= 4096
    for module, name, value in RESTATED:
        assert getattr(importlib.import_module(f"tests.{module}"), name) == value, (module, name)


def test_every_macro_with_a_python_twin_agrees_with_it(c_values):
    for macro, twin, cases in MACROS:
        for args in cases:
            assert twin(*args) == c_values[_call(macro, args)], (macro, args)
    ws = _cabi.lp_components_frames_ws_bytes
    assert c_values["LP_COMPONENTS_FRAMES_WS_BYTES(1, 720, 1280)"] == c_values["LP_COMPONENTS_WS_BYTES(720, 1280)"]
    assert ws(1, 1, 1) == 4100 and ws(3, 17, 65) == _cabi.lp_components_ws_bytes(51, 65)
    assert _cabi.lp_color_ws_bytes(81, 576, 1024, 3) == 81 * 18 * 8 * 13 * 8       # one partial row per 32 x 128 tile
    assert c_values["LP_PROP_MATCH_GATED(16)"] == 4097


def test_the_abi_version_is_25_in_the_header_the_mirror_and_the_library(hip_lib, c_values):
    assert c_values["LP_ABI_VERSION"] == _cabi.ABI_VERSION == hip_lib.lp_abi_version() == 25


def test_the_version_script_exports_exactly_the_lp_names(hip_lib):
    script = open(os.path.join(ROOT, "lanpaint_amd", "csrc", "exports.map")).read()
    assert [p.split() for p in re.findall(r"global:\s*([^;]+);", script)] == [["lp_*"]]
    dynamic = subprocess.run(["nm", "-D", "--defined-only", _cabi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(re.findall(r"\bT (\w+)$", dynamic, flags=re.M)) == sorted(HEADER.functions)      # every entry a function, `T`


def _modules():
    return sorted(glob.glob(os.path.join(ROOT, "lanpaint_amd", "*.py")))


def test_no_module_of_the_package_reads_an_unbound_name():
    files = _modules()
    assert len(files) >= 68
    files.append(os.path.join(ROOT, "scripts", "bench_propagate_anchored_visible.py"))      # the one script a per-module test named
    p = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_names.py"), *files], capture_output=True, text=True)
    assert p.returncode == 0 and f"{len(files)} files" in p.stdout, p.stdout


def test_every_node_module_keeps_the_protocol_and_no_two_share_a_name():
    names = [os.path.basename(f)[:-3] for f in _modules() if "nodes" in os.path.basename(f)]
    modules = [m for m in (importlib.import_module(f"lanpaint_amd.{n}") for n in names) if hasattr(m, "NODE_CLASS_MAPPINGS")]
    assert len(modules) >= 26
    for m in modules:
        assert set(m.NODE_DISPLAY_NAME_MAPPINGS) == set(m.NODE_CLASS_MAPPINGS) and m.NODE_CLASS_MAPPINGS, m.__name__
        for key, cls in m.NODE_CLASS_MAPPINGS.items():
            assert key.startswith("LanPaint_"), key
            assert callable(getattr(cls, cls.FUNCTION)) and cls.CATEGORY and "required" in cls.INPUT_TYPES(), key
            assert not hasattr(cls, "RETURN_NAMES") or len(cls.RETURN_NAMES) == len(cls.RETURN_TYPES), key
    keys = [(key, m.__name__) for m in modules for key in m.NODE_CLASS_MAPPINGS]
    shown = [(text, m.__name__) for m in modules for text in m.NODE_DISPLAY_NAME_MAPPINGS.values()]
    for owners in (keys, shown):                                      # no two alike, within a module or across any two
        seen = [entry for entry, _ in owners]
        assert len(seen) >= 50 and not [o for o in owners if seen.count(o[0]) > 1]
