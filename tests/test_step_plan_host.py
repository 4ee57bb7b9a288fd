"""csrc/step_plan.h on the CPU: tools/step_plan_host_check.cpp built with a host compiler alone and run (no GPU, no HIP),
and a look through the sources for what the plan, the step state and the lookahead functions replaced."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphem-rapids_amd", "csrc")


def test_step_plan_host_check(tmp_path):
    cxx = shutil.which(os.environ.get("HOSTCXX", "g++")) or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "step_plan_host_check")
    build = subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tools", "step_plan_host_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "step_plan_host_check: ok" in run.stdout


def _sources():
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h", ".cpp")):
            with open(os.path.join(CSRC, name)) as f:
                yield name, f.read()


def test_lookahead_only_through_its_functions():
    users = [name for name, text in _sources() if "lookahead." in text and name not in ("engine.h", "step_plan.h")]
    assert users == []


# functions that the plan replaced, and members of gh_engine that the plan, the requests and the step state replaced
REMOVED_FUNCTIONS = ["gh_knn_scan_path", "gh_grid_path", "gh_ivf_path", "gh_fused_uses_mfma", "gh_fused_mfma_kb", "gh_fused_cells_ok",
                     "gh_coarse_tau_ok", "gh_choose_scan_filter", "gh_choose_threshold_subset", "gh_fused_tile", "fused_cfg",
                     "fused_mfma", "fused_mfma_kb", "subset_stride"]
REMOVED_MEMBERS = ["qcells", "tau_embedded", "tau_embedded_plan", "coarse_tau", "coarse_mode", "scan_filter", "opt_no_presetup",
                   "thr_stride", "thr_M1", "last_step_own_ids",
                   # the exchange of a partitioned step: now h->xch, its layout value made by csrc/exchange_layout.h
                   "d_gbuf", "g_slot", "g_chunk", "g_world", "g_rank", "layout", "d_rows_packed", "packed_exchange", "d_rows_all",
                   "d_rows_pk", "d_stats_all", "stats_block", "patch_cap",
                   # the step flags: now in h->step, written through the gh_step_* functions of engine.h
                   "new0_ready", "intersect_done", "stats_reduced", "tcount_reset_pending", "rows_early"]
STEP_FLAGS = REMOVED_MEMBERS[-5:] + ["own_ids"]


def test_removed_names_are_gone():
    found = []
    for name, text in _sources():
        code = re.sub(r"//[^\n]*|/\*.*?\*/", "", text, flags=re.S)   # (comments may tell the history)
        found += [(name, word) for word in REMOVED_FUNCTIONS if re.search(r"(?<!\w)" + word + r"\s*\(", code)]
        found += [(name, "->" + word) for word in REMOVED_MEMBERS if re.search(r"\bh->" + word + r"\b", code)]
        if name != "engine.h":
            found += [(name, "write to step." + flag) for flag in STEP_FLAGS if re.search(r"step\." + flag + r"\s*=[^=]", code)]
            # (gh_cmin_claim in fused.hip and gh_cmin_release in engine.h are the two writers)
            if name != "fused.hip" and re.search(r"cmin_dirty\[[^\]]*\]\s*=[^=]", code):
                found.append((name, "write to cmin_dirty"))
    assert found == []
