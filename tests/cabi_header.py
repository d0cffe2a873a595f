"""include/lanpaint_hip.h as data, for tests/test_cabi_mirror.py: its structs, its LP_API prototypes and its object-like LP_* macros,
read with regular expressions that know exactly the declaration shapes the header uses.  A declaration of another shape raises
with its text: nothing is skipped.  `_call` and `_signed` serve the tests that hand the header's macros to a C compiler."""
import collections
import keyword
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lanpaint_hip.h")

# `const float* x`, `void* const* x`, `const struct lp_graph_binding* const* x`, `uint32_t grid[3]`, `float* x0s_buf[LP_N]`:
# `base` without const / struct, `ptr` the number of stars, `length` None for what is no array
Field = collections.namedtuple("Field", "base ptr name length")
Function = collections.namedtuple("Function", "result name args")
Header = collections.namedtuple("Header", "structs functions defines")

_TYPE = re.compile(r"(?:const\s+)?(?:struct\s+)?([A-Za-z_]\w*)\b\s*(.*)", re.S)
_DECLARATOR = re.compile(r"((?:\*\s*(?:const\b\s*)?)*)([A-Za-z_]\w*)?\s*(?:\[\s*(\w+)\s*\])?")


def _declaration(text, constants, named=True):
    """`type declarator, declarator ...` -> one Field per declarator (the stars belong to the declarator, as in C)."""
    m = _TYPE.fullmatch(text.strip())
    fields = []
    for part in m.group(2).split(",") if m else []:
        d = _DECLARATOR.fullmatch(part.strip())
        if d is None or bool(d.group(2)) != named:
            raise ValueError(f"cannot read the declaration: {text.strip()!r}")
        length = d.group(3)
        if length is not None:
            length = int(length) if length.isdigit() else constants[length]
        fields.append(Field(m.group(1), d.group(1).count("*"), d.group(2) or "", length))
    if not fields:
        raise ValueError(f"cannot read the declaration: {text.strip()!r}")
    return fields


def parse(path=HEADER):
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src).replace("\\\n", " ")
    defines, constants = [], {}
    for name, params, body in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(LP_\w+)(\()?[ \t]*(.*)$", src, flags=re.M):
        if not params:                                       # object-like; LP_FOO(x) is function-like
            defines.append(name)
            if re.fullmatch(r"\d+", body.strip()):
                constants[name] = int(body)
    structs = collections.OrderedDict()
    for tag, body, name in re.findall(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", src, flags=re.S):
        if tag != name or name in structs or "{" in body:
            raise ValueError(f"cannot read the struct: {tag} / {name}")
        structs[name] = [f for decl in body.split(";") if decl.strip() for f in _declaration(decl, constants)]
    functions = collections.OrderedDict()
    for proto in re.findall(r"\bLP_API\b(?!\s+__attribute__)([^;{]*);", src):
        m = re.fullmatch(r"\s*(.*?)\b(lp_\w+)\s*\((.*)\)\s*", proto, flags=re.S)
        if m is None or m.group(2) in functions:
            raise ValueError(f"cannot read the prototype: LP_API{proto!r}")
        args = [] if m.group(3).strip() == "void" else [_declaration(a, constants)[0] for a in m.group(3).split(",")]
        functions[m.group(2)] = Function(_declaration(m.group(1), constants, named=False)[0], m.group(2), args)
    if len(re.findall(r"\btypedef\b", src)) != len(structs) or len(re.findall(r"\bLP_API\b", src)) != len(functions) + 1:
        raise ValueError("a typedef or an LP_API of the header was not read")        # + 1: the #define of LP_API itself
    return Header(structs, functions, defines)


def class_name(c_name):
    """lp_prop_match_job -> LpPropMatchJob"""
    return "".join(w.capitalize() for w in c_name.split("_"))


def field_name(c_name):
    """The Python field is the C field, plus a trailing underscore where that is a keyword (lambda -> lambda_)."""
    return c_name + "_" if keyword.iskeyword(c_name) else c_name


def _call(macro, args):
    return "%s(%s)" % (macro, ", ".join(map(str, args)))


def _signed(u):
    return u - (1 << 32) if u >= 1 << 31 else u
