#!/usr/bin/env python3
"""Record what a float32 engine launches and computes over a fixed script of steps, case by case.

    python tools/record_step_launches.py [--which all|single|partitioned] [--out FILE] [--out-partitioned FILE] [--check]

Every case creates an engine, enables timing and runs: set positions; three steps with the engine's own ids; one step with
given ids; one step with own ids; knn_midpoints with given ids.  Recorded per case: {timer slot: launches}, the SHA-256 of
the positions after each of the five steps, the SHA-256 of the neighbour rows, the pre-filter and threshold form in use at
the end, and the SHA-256 of the candidate counts of the last search.  tests/test_hip_step_plan.py compares a run of the
current build with the committed record, which pins the choice of launches and the results across refactors of the host
code.  --check: run every case twice and report cases whose two records differ (nothing is written for them).

Uses only timing_enable, timings, scan_filter, coarse_tau and knn_last_counts besides the stepping calls.

PARTITIONED_CASES (--out-partitioned, tests/golden/partitioned_step_launches.json) do the same for the row-partitioned step:
`world` engines on one GPU in one process, driven by distributed.step_in_process or, the `native` cases, by
gh_run_partitioned over the loopback backend with one thread per rank.  Recorded per rank: {timer slot: launches} and the
SHA-256 of its positions after each of the same five steps; for a case the library refuses, the exception and its message."""
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


# name -> finish ("gathered": form B, "own": form C, "overlap": form D), world and what differs from the defaults above.
# packed: form C's unpadded block exchange forced on / off; ownership: "hashed" unless said; native: gh_run_partitioned.
PARTITIONED_CASES = {
    "b_w2": {"finish": "gathered", "world": 2},
    "b_w3": {"finish": "gathered", "world": 3},                  # (world 3: a ragged last block)
    "c_w2_packed": {"finish": "own", "world": 2, "packed": True},
    "c_w2_unpacked": {"finish": "own", "world": 2, "packed": False},
    "c_w3_packed": {"finish": "own", "world": 3, "packed": True},
    "c_w3_unpacked": {"finish": "own", "world": 3, "packed": False},
    "d_w2": {"finish": "overlap", "world": 2},
    "d_w3": {"finish": "overlap", "world": 3},
    "c_d5_w2": {"finish": "own", "world": 2, "D": 5, "packed": True},       # stride 8, packed
    "d_d5_w2": {"finish": "overlap", "world": 2, "D": 5},
    "c_d16_w2": {"finish": "own", "world": 2, "D": 16},                     # stride 16: nothing to pack
    "d_d16_w2": {"finish": "overlap", "world": 2, "D": 16},
    "b_d20_w2": {"finish": "gathered", "world": 2, "D": 20},                # stride above 16: the generic kernels
    "c_d20_w2": {"finish": "own", "world": 2, "D": 20},
    "d_d20_refused": {"finish": "overlap", "world": 2, "D": 20},            # form D takes up to 16 floats of stride
    "d_n2000_w2": {"finish": "overlap", "world": 2, "n": 2000},             # no fused kernel: new0 from its own launch
    "d_range_w2": {"finish": "overlap", "world": 2, "ownership": "range"},
    "native_b_w2": {"finish": "gathered", "world": 2, "native": True},
    "native_c_w2": {"finish": "own", "world": 2, "native": True},
    "native_d_w2": {"finish": "overlap", "world": 2, "native": True},
    "d_empty_last_rank": {"finish": "overlap", "world": 4, "n": 9},         # chunk 3: rank 3 owns no rows
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


def record_partitioned_case(name):
    import threading

    import torch

    import graphem_rapids_amd as gra
    from graphem_rapids_amd import _native
    from graphem_rapids_amd.distributed import HipShardEngine, partition_edges, partition_rows, step_in_process
    c = PARTITIONED_CASES[name]
    n, D, k, world, finish = c.get("n", 20000), c.get("D", 3), 10, c["world"], c["finish"]
    if n < 16:   # a ring with chords: enough edges for k + 1 keys
        ring = np.arange(n)
        edges = np.concatenate([np.stack([ring, (ring + s) % n], axis=1) for s in (1, 2)])
        edges = np.unique(np.sort(edges, axis=1), axis=0).astype(np.int32)
    else:
        edges = gra.random_regular_edges(n, 8, seed=0).astype(np.int32)
    S = min(256, len(edges))
    rng = np.random.default_rng(0)
    pos = (rng.standard_normal((n, D)) * 0.1).astype(np.float32)
    ids_step = rng.permutation(len(edges))[:S].astype(np.int32)
    lib = _native.load()
    group = lib.gh_loopback_group_create(world) if c.get("native") else None
    shards = []
    try:
        for r in range(world):
            chunk, lo, hi = partition_rows(n, world, r)
            if c.get("ownership", "hashed") == "hashed":
                part = (lo, hi, 0, 0, _native.EDGES_HASHED)
            else:
                part = (lo, hi, *partition_edges(edges, lo, hi), _native.EDGES_RANGE)
            sh = HipShardEngine(n, D, edges, 1.0, 0.2, 0.5, k, S, 0, part, 0)
            shards.append(sh)
            if finish == "own":
                sh.rank_layout(world, r, chunk, packed=c.get("packed"))
            elif finish == "overlap":
                sh.overlap_layout(world, r, chunk)
            else:
                sh.gather_layout(world, r, chunk)
            if group is not None:
                sh.eng.set_stream(0, use_own=True)
                sh.eng.comm_init_loopback(group, r)
            sh.eng.timing_enable(True)
            sh.set_positions(pos)
        positions = [[] for _ in shards]
        for step in range(5):
            ids = ids_step if step == 3 else None
            if group is None:
                step_in_process(shards, finish, ids)
                torch.cuda.synchronize()
            else:
                errors = []

                def work(sh):
                    try:
                        sh.run_partitioned(1, None if ids is None else ids[None, :])
                    except Exception as exc:  # pylint: disable=broad-exception-caught
                        errors.append(exc)
                threads = [threading.Thread(target=work, args=(sh,)) for sh in shards]
                for t in threads:
                    t.start()
                for t in threads:
                    t.join(timeout=120)
                if errors or any(t.is_alive() for t in threads):
                    raise RuntimeError(f"native step failed: {errors}")
            for r, sh in enumerate(shards):
                positions[r].append(sha(sh.get_positions()))
        for sh in shards:
            sh.sync()
        return {"ranks": [{"launches": {slot: int(cnt) for slot, (_, cnt) in sorted(sh.eng.timings().items())},
                           "positions": positions[r]} for r, sh in enumerate(shards)]}
    except (ValueError, RuntimeError, MemoryError) as exc:   # the library's refusal: its status (as the exception) and message
        return {"refused": [type(exc).__name__, str(exc)]}
    finally:
        for sh in shards:
            if group is not None:
                try:
                    sh.eng.comm_destroy()
                except (ValueError, RuntimeError):
                    pass
            sh.eng.close()
        if group is not None:
            lib.gh_loopback_group_destroy(group)


def record_all(cases, record, path, check):
    out, unstable = {}, []
    for name in cases:
        rec = record(name)
        if check and record(name) != rec:
            unstable.append(name)
            continue
        out[name] = rec
        if "refused" in rec:
            print(f"{name}: refused: {rec['refused']}", flush=True)
            continue
        per_rank = rec["ranks"] if "ranks" in rec else [rec]
        print(f"{name}: {[sum(r['launches'].values()) for r in per_rank]} launches"
              + (f", filter {rec['scan_filter']}, coarse {rec['coarse_tau']}" if "ranks" not in rec else ""), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(out)} cases to {path}" + (f"; NOT reproducible: {unstable}" if unstable else ""))
    return unstable


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "step_launches.json"))
    ap.add_argument("--out-partitioned", default=os.path.join(ROOT, "tests", "golden", "partitioned_step_launches.json"))
    ap.add_argument("--which", choices=("all", "single", "partitioned"), default="all", help="the set of cases to record")
    ap.add_argument("--check", action="store_true", help="run every case twice; report and leave out cases that differ")
    args = ap.parse_args()
    unstable = []
    if args.which in ("all", "single"):
        unstable += record_all(CASES, record_case, args.out, args.check)
    if args.which in ("all", "partitioned"):
        unstable += record_all(PARTITIONED_CASES, record_partitioned_case, args.out_partitioned, args.check)
    return 1 if unstable else 0


if __name__ == "__main__":
    sys.exit(main())
