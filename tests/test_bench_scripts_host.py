"""The feature benchmarks (scripts/bench_*.py) measure through one kit, scripts/featurebench.py: the structure of the scripts, read
from their syntax trees and by importing them without a device, and the kit's series, spread and format helpers on a fake clock."""
import ast
import glob
import importlib
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "scripts")
BENCHES = sorted(os.path.basename(p)[:-3] for p in glob.glob(os.path.join(SCRIPTS, "bench_*.py")))
TIMER_NAMES = {"wall", "events", "timed", "count_launches"}


@pytest.fixture
def no_device(monkeypatch):
    import torch
    monkeypatch.syspath_prepend(SCRIPTS)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)


@pytest.fixture
def fb(no_device):
    return importlib.import_module("featurebench")


def _tree(name):
    with open(os.path.join(SCRIPTS, name + ".py")) as f:
        return ast.parse(f.read())


def test_there_are_benchmarks_to_check():
    assert len(BENCHES) >= 26 and "bench_propagate" in BENCHES


@pytest.mark.parametrize("name", BENCHES)
def test_script_imports_without_a_device_and_main_asks_for_one(name, no_device, monkeypatch):
    module = importlib.import_module(name)
    monkeypatch.setattr(sys, "argv", [os.path.join(SCRIPTS, name + ".py")])
    with pytest.raises(SystemExit) as stop:
        module.main()
    assert str(stop.value).startswith(f"{name}.py needs a HIP device")


@pytest.mark.parametrize("name", BENCHES)
def test_script_takes_its_times_from_the_kit(name):
    tree = _tree(name)
    defined = {n.name for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef))}
    assert not defined & TIMER_NAMES, defined & TIMER_NAMES
    for node in ast.walk(tree):
        if isinstance(node, ast.Attribute):
            assert not (node.attr == "Event" and isinstance(node.value, ast.Attribute) and node.value.attr == "cuda"), node.lineno
            assert node.attr != "perf_counter", node.lineno
        if isinstance(node, ast.ImportFrom):
            assert node.module != "time" and not (node.module or "").startswith("bench_"), node.lineno
        if isinstance(node, ast.Import):
            assert all(a.name != "time" for a in node.names), node.lineno
    assert any(isinstance(n, ast.Import) and any(a.name == "featurebench" for a in n.names) for n in ast.walk(tree))


@pytest.mark.parametrize("name", BENCHES)
def test_script_imports_another_benchmark_for_its_workload_only(name):
    tree = _tree(name)
    aliases = {(a.asname or a.name): a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names
               if a.name.startswith("bench_")}
    used = {alias: set() for alias in aliases}
    for node in ast.walk(tree):
        if isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name) and node.value.id in used:
            used[node.value.id].add(node.attr)
    for alias, names in used.items():
        assert names - TIMER_NAMES, f"{name} imports {aliases[alias]} and uses nothing of its workload"
        assert not names & TIMER_NAMES, f"{name} takes {sorted(names & TIMER_NAMES)} from {aliases[alias]}"


# ---- the kit on a fake clock ---------------------------------------------------------------------------------------------------
class Script:
    """A clock that reads a scripted sequence of times (seconds), and a log of what ran in which order."""

    def __init__(self, times):
        self.times, self.log = list(times), []

    def clock(self):
        self.log.append("clock")
        return self.times.pop(0)

    def sync(self):
        self.log.append("sync")

    def fn(self, tag):
        return lambda: self.log.append(tag)


def test_wall_reads_the_clock_inside_the_two_synchronises(fb):
    s = Script([10.0, 10.25])
    assert fb.wall(s.fn("call"), clock=s.clock, sync=s.sync) == 250.0
    assert s.log == ["sync", "clock", "call", "sync", "clock"]


def test_series_warms_up_untimed_then_interleaves_the_tags(fb):
    # three timed rounds of a, b, a: (start, end) per call, in seconds
    s = Script([0.0, 0.001, 1.0, 1.010, 2.0, 2.003,
                3.0, 3.002, 4.0, 4.030, 5.0, 5.001,
                6.0, 6.004, 7.0, 7.020, 8.0, 8.005])
    a, b = s.fn("a"), s.fn("b")
    rec = fb.series([("x_a", a), ("y", b), ("x_b", a)], iters=3, warmup=2, timer=lambda f: fb.wall(f, clock=s.clock, sync=s.sync), sync=s.sync)
    timed = ["sync", "clock", None, "sync", "clock"]
    want = ["a", "b", "a"] * 2 + ["sync"] + [tag if t is None else t for _ in range(3) for tag in ("a", "b", "a") for t in timed]
    assert s.log == want and not s.times
    assert list(rec) == ["x_a", "y", "x_b"]
    assert rec["x_a"] == pytest.approx([1.0, 2.0, 4.0]) and rec["y"] == pytest.approx([10.0, 30.0, 20.0])
    assert rec["x_b"] == pytest.approx([3.0, 1.0, 5.0])
    # medians 2 and 3, the median of all six 2.5: the spread is their relative difference
    assert fb.spread(rec["x_a"], rec["x_b"]) == 0.4
    assert fb.summary(rec["x_a"] + rec["x_b"]) == (2.5, [1.0, 5.0])
    assert fb.summary(rec["y"], 3) == (20.0, [10.0, 30.0])


def test_series_takes_a_timer_of_its_own_per_entry_and_none_at_zero_iterations(fb):
    log = []
    rec = fb.series([("w", lambda: log.append("w"), lambda f: (f(), 7.0)[1]), ("e", lambda: log.append("e"))], 2, 0,
                    timer=lambda f: (f(), 1.0)[1], sync=lambda: log.append("sync"))
    assert rec == {"w": [7.0, 7.0], "e": [1.0, 1.0]} and log == ["sync", "w", "e", "w", "e"]
    log.clear()
    assert fb.series([("w", lambda: log.append("w"))], 0, 3, sync=lambda: log.append("sync")) == {"w": []}
    assert log == ["w", "w", "w", "sync"]


def test_spread_and_summary_round_as_the_json_lines_do(fb):
    a, b = [1.00004, 1.00016, 1.2], [0.9, 1.00026, 1.00035]
    # medians 1.00016 and 1.00026 over the median of the six, (1.00016 + 1.00026) / 2
    assert fb.spread(a, b) == round(0.0001 / 1.00021, 4) == 0.0001
    assert fb.spread(a, b, 6) == round(0.0001 / 1.00021, 6)
    assert fb.summary(a) == (1.0002, [1.0, 1.2])
    assert fb.summary(a, 3) == (1.0, [1.0, 1.2])
    assert fb.summary([2.0, 1.0], 3) == (1.5, [1.0, 2.0])


def test_parser_device_and_line(fb, monkeypatch, capsys):
    import torch
    a = fb.parser({"clip": 1, "square": 2}, ("whole",), iters=5, warmup=1).parse_args(["--case", "square"])
    assert (a.iters, a.warmup, a.case, a.job) == (5, 1, "square", None)
    assert not hasattr(fb.parser(iters=30, warmup=5).parse_args([]), "case")
    monkeypatch.setattr(sys, "argv", ["scripts/bench_x.py"])
    with pytest.raises(SystemExit, match=r"^bench_x\.py needs a HIP device$"):
        fb.device()
    monkeypatch.setattr(torch.cuda, "get_device_name", lambda i: "a device")
    fb.emit("m", a, [{"case": "square"}], extra=True)
    assert capsys.readouterr().out == '{"metric":"m","unit":"ms","device":"a device","iters":5,"warmup":1,"cases":[{"case":"square"}],"extra":true}\n'
