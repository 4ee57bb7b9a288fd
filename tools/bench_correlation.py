"""Times one full correlation report (seven columns, the six pairs with the radii, 1000 bootstrap replicates, plus the
7 x 7 matrix) on the device path, on the library's host path, and with the reference's procedure (per replicate and
pair: draw n indices, scipy.stats.spearmanr on the two resampled arrays), restated here.

One warm-up call per size, then the median of 5 calls; a call includes making the handle (upload and sort of the
columns) and the download of the replicates.  The reference's procedure is timed on fewer replicates where 6000 of them
would take hours, and the row says that its figure is extrapolated.  Prints one JSON line per size and appends it to
profiles/correlation/bench.jsonl.  Needs a GPU.

    python tools/bench_correlation.py
    python tools/bench_correlation.py --sizes 1000000 --calls 1 --no-baseline --no-host      e.g. under a profiler
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graphem_rapids_amd import _native  # noqa: E402

PAIRS = np.array([[0, j] for j in range(1, 7)], dtype=np.int32)


def columns(n):
    rng = np.random.default_rng(77)
    degree = np.floor(rng.pareto(2.0, n) * 2 + 1)
    radii = 5.0 / np.sqrt(degree) + rng.standard_normal(n) * 0.3
    btw = np.where(rng.random(n) < 0.8, 0.0, rng.random(n) * degree)
    eig = np.exp(rng.standard_normal(n)) * degree
    pr = degree / degree.sum() + rng.random(n) * 1e-9
    clo = np.round(0.2 + rng.standard_normal(n) * 0.01, 4)
    load = btw * 1.5 + np.where(btw > 0, rng.random(n), 0.0)
    return np.stack([radii, degree, btw, eig, pr, clo, load])


def report(cols, device_id, reps):
    corr = _native.Correlation(cols, device_id)
    corr.matrix()
    out = corr.bootstrap(PAIRS, reps, 0)
    corr.close()
    return out


def reference_procedure(cols, reps):
    from scipy import stats
    n = cols.shape[1]
    for j in range(1, 7):
        stats.spearmanr(cols[0], cols[j])
        for _ in range(reps):
            idx = np.random.choice(n, n, replace=True)
            stats.spearmanr(cols[0][idx], cols[j][idx])


def timed(fn, calls):
    fn()                                    # warm-up
    out = []
    for _ in range(calls):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,100000,1000000")
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "correlation", "bench.jsonl"))
    args = ap.parse_args()
    if _native.load().gh_device_count() < 1:
        sys.exit("bench_correlation.py needs a GPU")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for n in [int(s) for s in args.sizes.split(",")]:
        cols = columns(n)
        row = {"row": f"report_n{n}", "n": n, "columns": 7, "pairs": 6, "reps": args.reps}
        ms = timed(lambda: report(cols, 0, args.reps), args.calls)
        row["device_ms_median"], row["device_ms"] = round(statistics.median(ms), 3), [round(x, 3) for x in ms]
        if not args.no_host:
            ms = timed(lambda: report(cols, -1, args.reps), args.calls)
            row["host_ms_median"], row["host_ms"] = round(statistics.median(ms), 3), [round(x, 3) for x in ms]
            row["host_threads"] = min(16, os.cpu_count() or 1)
        if not args.no_baseline:
            timed_reps = args.reps if n <= 10_000 else 20 if n <= 100_000 else 5
            t = time.perf_counter()
            reference_procedure(cols, timed_reps)
            seconds = time.perf_counter() - t
            row["reference_ms"] = round(seconds * 1e3 * args.reps / timed_reps, 1)
            row["reference_replicates_timed"] = timed_reps
            row["reference_extrapolated"] = timed_reps != args.reps
            row["speedup_vs_reference"] = round(row["reference_ms"] / row["device_ms_median"], 1)
        print(json.dumps(row), flush=True)
        with open(args.out, "a", encoding="utf-8") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
