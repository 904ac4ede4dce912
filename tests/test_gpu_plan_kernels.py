"""The forward planner launches the kernels it launched before: tests/golden/plan_kernels.json (recorded by
tests/golden/make_plan_golden.py from the commit BEFORE the planner was last changed) replayed on the library under test.

Per case -- precision x tuning flags x BiLSTM tiling x sites per forward -- the `(kernel name, launches)` pairs of
`kernel_stats()` and the `(name, launches, flops_per_site)` rows of `stage_times()` must be equal to the record: names and
counts exactly, FLOPs exactly (exact doubles on both sides). A variant booked under another kernel's name, a launch that
moved between stages, or a FLOP formula that changed shows up here; the numbers the kernels compute are the parity tests'."""
import functools
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN, "plan_kernels.json")) as _f:
    FIXTURE = json.load(_f)


@functools.lru_cache(maxsize=None)
def _generator():
    spec = importlib.util.spec_from_file_location("make_plan_golden", os.path.join(GOLDEN, "make_plan_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_holds_the_generators_cases():
    want = [{"id": cid, "engine": kw, "forwards": fw} for cid, kw, fw in _generator().cases()]
    assert [{k: c[k] for k in ("id", "engine", "forwards")} for c in FIXTURE["cases"]] == want


def test_cases_reach_every_kernel_a_forward_can_launch():
    gen = _generator()
    seen = {name for c in FIXTURE["cases"] for name, _ in c["kernels"]}
    assert set(FIXTURE["kernel_table"]) - seen == gen.NEVER_LAUNCHED


@pytest.mark.gpu
@pytest.mark.parametrize("case", FIXTURE["cases"], ids=[c["id"] for c in FIXTURE["cases"]])
def test_planner_launches_the_recorded_kernels(case):
    kernels, stages, names = _generator().replay(case["engine"], case["forwards"])
    assert names == FIXTURE["kernel_table"]          # order, count and names of the kernel table (ds_get_kernel_stat is ABI)
    assert kernels == case["kernels"]
    assert stages == case["stages"]
