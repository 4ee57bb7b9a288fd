#!/usr/bin/env python3
"""Record what a float32 engine launches and computes over a fixed script of steps, case by case.

    python tools/record_step_launches.py [--out tests/golden/step_launches.json] [--check]

Every case creates an engine, enables timing and runs: set positions; three steps with the engine's own ids; one step with
given ids; one step with own ids; knn_midpoints with given ids.  Recorded per case: {timer slot: launches}, the SHA-256 of
the positions after each of the five steps, the SHA-256 of the neighbour rows, the pre-filter and threshold form in use at
the end, and the SHA-256 of the candidate counts of the last search.  tests/test_hip_step_plan.py compares a run of the
current build with the committed record, which pins the choice of launches and the results across refactors of the host
code.  --check: run every case twice and report cases whose two records differ (nothing is written for them).

Uses only timing_enable, timings, scan_filter, coarse_tau and knn_last_counts besides the stepping calls."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# name -> engine arguments and requests.  Defaults: n = 20000 (random_regular_edges(n, 8)), D = 3, S = 256, k = 10.
# env: set before the engine is created; filter / coarse: set right after; switch: (filter, coarse) set between steps 2 and 3.
CASES = {
    "default_d3": {},
    "d2": {"D": 2},
    "d6": {"D": 6},
    "tau_separate": {"env": {"GRAPHEM_HIP_TAU_SEPARATE": "1"}},
    "cells_coarse_off": {"filter": "cells", "coarse": "off"},
    "cells_coarse_on": {"filter": "cells", "coarse": "on"},
    "mfma": {"filter": "mfma"},
    "k31_cells_coarse_on": {"k": 31, "filter": "cells", "coarse": "on"},
    "k40_cells": {"k": 40, "filter": "cells", "coarse": "on"},   # (more keys than the coarse form bounds: stays off)
    "cdist": {"knn_distance": "cdist"},
    "grid": {"knn_method": "grid"},
    # (counts: the lengths of the IVF search's candidate lists vary from run to run -- its thresholds tighten in the order
    # the workgroups of a launch happen to finish -- while rows and positions do not: the lengths are left out)
    "ivf_all_probes": {"knn_method": "ivf", "ivf_probes": -1, "counts": False},
    "s2048": {"S": 2048},
    "k128": {"k": 128},
    "n2000_exhaustive": {"n": 2000},
    "no_presetup": {"env": {"GRAPHEM_HIP_NO_PRESETUP": "1"}},
    "switch_between_steps": {"switch": ("cells", "on")},
}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def record_case(name):
    import graphem_rapids_amd as gra
    from graphem_rapids_amd import _native
    c = CASES[name]
    n, D, S, k = c.get("n", 20000), c.get("D", 3), c.get("S", 256), c.get("k", 10)
    edges = gra.random_regular_edges(n, 8, seed=0).astype(np.int32)
    rng = np.random.default_rng(0)
    pos = (rng.standard_normal((n, D)) * 0.1).astype(np.float32)
    ids_step = rng.permutation(len(edges))[:S].astype(np.int32)
    ids_knn = rng.permutation(len(edges))[:S].astype(np.int32)
    env = c.get("env", {})
    saved = {key: os.environ.get(key) for key in env}
    os.environ.update(env)
    try:
        eng = _native.Engine(n, D, edges, 1.0, 0.2, 0.5, k, S, knn_method=c.get("knn_method", "auto"),
                             knn_distance=c.get("knn_distance", "exact"), ivf_probes=c.get("ivf_probes", 0))
    finally:
        for key, val in saved.items():
            if val is None:
                os.environ.pop(key, None)
            else:
                os.environ[key] = val
    try:
        eng.timing_enable(True)
        if "filter" in c:
            eng.set_scan_filter(c["filter"])
        if "coarse" in c:
            eng.set_coarse_tau(c["coarse"])
        eng.set_positions(pos)
        positions = []
        for step in range(5):
            if step == 2 and "switch" in c:
                eng.set_scan_filter(c["switch"][0])
                eng.set_coarse_tau(c["switch"][1])
            eng.step(ids_step if step == 3 else None)
            positions.append(sha(eng.get_positions()))
        rows = eng.knn_midpoints(ids_knn)
        eng.sync()
        counts = eng.knn_last_counts()
        return {
            "launches": {slot: int(cnt) for slot, (_, cnt) in sorted(eng.timings().items())},
            "positions": positions,
            "knn_rows": sha(rows),
            "knn_counts": [sha(a) for a in counts] if c.get("counts", True) else None,
            "scan_filter": eng.scan_filter(),
            "coarse_tau": bool(eng.coarse_tau()),
        }
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "step_launches.json"))
    ap.add_argument("--check", action="store_true", help="run every case twice; report and leave out cases that differ")
    args = ap.parse_args()
    out, unstable = {}, []
    for name in CASES:
        rec = record_case(name)
        if args.check and record_case(name) != rec:
            unstable.append(name)
            continue
        out[name] = rec
        print(f"{name}: {sum(rec['launches'].values())} launches in {len(rec['launches'])} slots, "
              f"filter {rec['scan_filter']}, coarse {rec['coarse_tau']}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(out)} cases to {args.out}" + (f"; NOT reproducible: {unstable}" if unstable else ""))
    return 1 if unstable else 0


if __name__ == "__main__":
    sys.exit(main())
