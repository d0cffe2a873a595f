"""The layout of the suite itself, read from the syntax trees of tests/*.py and of the generators under tests/golden/: what more than
one test module uses lives in plain helper modules, once.  No test module is imported by another module, no helper module defines
a test, no function is defined twice, and the numpy-only helper modules stay free of torch and of the product package."""
import ast
import glob
import os

TESTS = os.path.dirname(os.path.abspath(__file__))
# comparisons, inputs and scenes: numpy and the *_ref restatements only, so that a host test's imports reach no device code
NUMPY_ONLY = ["compare", "inputs", "image_inputs", "propagate_scenes", "temporal_clips", "anchor_clips", "shot_clips", "focus_scenes"]


def _sources():
    paths = sorted(glob.glob(os.path.join(TESTS, "*.py")) + glob.glob(os.path.join(TESTS, "golden", "*.py")))
    out = {}
    for path in paths:
        with open(path) as f:
            out[os.path.relpath(path, TESTS)] = f.read()
    return out


def _is_helper(name):
    base = os.path.basename(name)
    return os.path.dirname(name) == "" and not base.startswith("test_") and base != "conftest.py"


def imports_of_test_modules(source):
    """(line, module) of every import of a tests.test_* module, at any depth."""
    found = []
    for node in ast.walk(ast.parse(source)):
        if isinstance(node, ast.Import):
            found += [(node.lineno, a.name) for a in node.names if a.name.startswith("tests.test_")]
        elif isinstance(node, ast.ImportFrom) and node.level == 0:
            module = node.module or ""
            if module.startswith("tests.test_"):
                found.append((node.lineno, module))
            elif module == "tests":
                found += [(node.lineno, "tests." + a.name) for a in node.names if a.name.startswith("test_")]
    return found


def definitions_of_tests(source):
    """Names of the functions and classes, at any depth, that pytest would take for tests."""
    return [node.name for node in ast.walk(ast.parse(source))
            if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)) and node.name.startswith(("test", "Test"))]


def _function_keys(source):
    """name -> (name, arguments, body without its docstring) of every module-level function."""
    keys = {}
    for node in ast.parse(source).body:
        if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)):
            body = node.body
            if body and isinstance(body[0], ast.Expr) and isinstance(body[0].value, ast.Constant) and isinstance(body[0].value.value, str):
                body = body[1:]
            keys[node.name] = (node.name, ast.dump(node.args), "".join(ast.dump(b) for b in body))
    return keys


def duplicated_functions(sources):
    """[(function name, the files that define it alike)]; the *_ref.py restatements are exempt among themselves."""
    seen = {}
    for name, source in sources.items():
        for key in _function_keys(source).values():
            seen.setdefault(key, []).append(name)
    out = []
    for key, files in seen.items():
        if len(files) > 1 and not all(f.endswith("_ref.py") for f in files):
            out.append((key[0], files))
    return out


def imported_roots(source):
    roots = set()
    for node in ast.walk(ast.parse(source)):
        if isinstance(node, ast.Import):
            roots |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom) and node.level == 0 and node.module:
            roots.add(node.module.split(".")[0])
    return roots


def test_no_module_imports_a_test_module():
    sources = _sources()
    assert len(sources) > 100 and "golden/make_golden.py" in sources and "test_gpu_propagate.py" in sources
    found = {name: imports_of_test_modules(source) for name, source in sources.items()}
    assert not {name: f for name, f in found.items() if f}


def test_helper_modules_define_no_tests():
    helpers = {name: source for name, source in _sources().items() if _is_helper(name)}
    assert {"compare.py", "inputs.py", "device.py", "helpers.py", "propagate_ref.py"} <= set(helpers) and "conftest.py" not in helpers
    found = {name: definitions_of_tests(source) for name, source in helpers.items()}
    assert not {name: f for name, f in found.items() if f}


def test_no_function_is_defined_twice():
    assert not duplicated_functions(_sources())


def test_the_numpy_kit_imports_no_device_code():
    sources = _sources()
    for module in NUMPY_ONLY:
        roots = imported_roots(sources[module + ".py"])
        assert not roots & {"torch", "lanpaint_amd"}, (module, sorted(roots))


def test_the_checks_find_what_they_look_for():
    nested = "import numpy as np\n\ndef f():\n    if True:\n        from tests.test_x import y\n    return y\n"
    assert imports_of_test_modules(nested) == [(5, "tests.test_x")]
    assert imports_of_test_modules("from tests import helpers, test_x as t\nimport tests.test_y\n") == [(1, "tests.test_x"), (2, "tests.test_y")]
    assert imports_of_test_modules("from tests.helpers import a\nfrom tests import poison\nimport tests.stubs\n") == []
    assert definitions_of_tests("def helper():\n    pass\n\ndef test_it():\n    pass\n\nclass TestThing:\n    pass\n") == ["test_it", "TestThing"]
    assert definitions_of_tests("def attest():\n    pass\n\nclass Contest:\n    pass\n") == []
    one = 'def _bits(a):\n    """One docstring."""\n    return a.view("u4")\n'
    two = 'import numpy\n\ndef _bits(a):\n    return a.view("u4")\n'
    other = 'def _bits(a):\n    return a.astype("f4").view("u4")\n'
    assert duplicated_functions({"test_a.py": one, "kit.py": two, "test_c.py": other}) == [("_bits", ["test_a.py", "kit.py"])]
    assert duplicated_functions({"test_a.py": one, "test_c.py": other}) == []
    assert duplicated_functions({"a_ref.py": one, "b_ref.py": two}) == []
    assert duplicated_functions({"a_ref.py": one, "b_ref.py": two, "test_a.py": two}) == [("_bits", ["a_ref.py", "b_ref.py", "test_a.py"])]
    assert imported_roots("import torch.nn\nfrom lanpaint_amd import _cabi\n\ndef f():\n    import numpy as np\n") == {"torch", "lanpaint_amd", "numpy"}
    assert _is_helper("compare.py") and not _is_helper("test_x.py") and not _is_helper("conftest.py") and not _is_helper("golden/make_golden.py")
