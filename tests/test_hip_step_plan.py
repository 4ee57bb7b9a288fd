"""The launches and results of a fixed script of steps, pinned case by case to tests/golden/step_launches.json, which
tools/record_step_launches.py recorded before the choice of path moved into csrc/step_plan.h: per case the launches of
every timer slot, the positions after each of five steps, the neighbour rows of a search behind them, the pre-filter and
the threshold form in use.  A host-side change that adds, drops or swaps a launch, or moves a result by a bit, fails here.
The partitioned forms are pinned by test_hip_parity.py and test_hip_multiproc.py."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorder():
    spec = importlib.util.spec_from_file_location("record_step_launches", os.path.join(ROOT, "tools", "record_step_launches.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


RECORDER = _recorder()
with open(os.path.join(ROOT, "tests", "golden", "step_launches.json")) as f:
    GOLDEN = json.load(f)


def test_every_case_is_recorded():
    assert sorted(GOLDEN) == sorted(RECORDER.CASES)


@pytest.mark.parametrize("name", sorted(RECORDER.CASES))
def test_launches_and_results_match_the_record(name):
    got, want = RECORDER.record_case(name), GOLDEN[name]
    assert got["launches"] == want["launches"]
    assert got["scan_filter"] == want["scan_filter"] and got["coarse_tau"] == want["coarse_tau"]
    for step, (a, b) in enumerate(zip(got["positions"], want["positions"])):
        assert a == b, f"positions after step {step + 1} differ from the record"
    assert len(got["positions"]) == len(want["positions"]) == 5
    assert got["knn_rows"] == want["knn_rows"]
    assert got["knn_counts"] == want["knn_counts"]
