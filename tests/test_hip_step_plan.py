"""The launches and results of a fixed script of steps, pinned case by case to tests/golden/step_launches.json, which
tools/record_step_launches.py recorded before the choice of path moved into csrc/step_plan.h: per case the launches of
every timer slot, the positions after each of five steps, the neighbour rows of a search behind them, the pre-filter and
the threshold form in use.  A host-side change that adds, drops or swaps a launch, or moves a result by a bit, fails here.
The partitioned forms are pinned the same way by tests/golden/partitioned_step_launches.json, recorded before their exchange
state moved into csrc/exchange_layout.h: per rank the launches of every timer slot and the positions after each of the five
steps, or the refusal the library gives."""
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
with open(os.path.join(ROOT, "tests", "golden", "partitioned_step_launches.json")) as f:
    GOLDEN_PARTITIONED = json.load(f)


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


def test_every_partitioned_case_is_recorded():
    assert sorted(GOLDEN_PARTITIONED) == sorted(RECORDER.PARTITIONED_CASES)
    for finish in ("gathered", "own", "overlap"):   # every form keeps a pinned run at world 2
        assert any(c["finish"] == finish and c["world"] == 2 and "ranks" in GOLDEN_PARTITIONED[name]
                   for name, c in RECORDER.PARTITIONED_CASES.items())


@pytest.mark.parametrize("name", sorted(RECORDER.PARTITIONED_CASES))
def test_partitioned_launches_and_results_match_the_record(name):
    got, want = RECORDER.record_partitioned_case(name), GOLDEN_PARTITIONED[name]
    assert got.get("refused") == want.get("refused")
    assert len(got.get("ranks", [])) == len(want.get("ranks", []))
    for rank, (g, w) in enumerate(zip(got.get("ranks", []), want.get("ranks", []))):
        assert g["launches"] == w["launches"], f"rank {rank}"
        assert len(g["positions"]) == len(w["positions"]) == 5
        for step, (a, b) in enumerate(zip(g["positions"], w["positions"])):
            assert a == b, f"rank {rank}: positions after step {step + 1} differ from the record"
