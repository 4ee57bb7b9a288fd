"""Layout quality of a generated graph before and after run_layout, and the time the counting takes.

    python tools/layout_quality.py --n 100000 --iters 20 --time [--host]

Prints layout_quality() of a random-regular graph's start and of its layout after --iters iterations.  --time measures,
on the final layout: the exact count over all edges, the estimate from --sample-size sampled edges, and with --host the
library's host path on the same snapshot (the only comparator there is).  Times are host clocks around blocking calls
(every call ends in a stream synchronise), after one warm-up call; one JSON line at the end.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import graphem_rapids_amd as gr   # noqa: E402
from graphem_rapids_amd import _native   # noqa: E402


def timed(fn, repeats):
    out, times = None, []
    for _ in range(repeats):
        t = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t)
    return out, min(times), times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--degree", type=int, default=8)
    ap.add_argument("--dim", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sample-size", type=int, default=4096)
    ap.add_argument("--exact", default=None, choices=["yes", "no"], help="layout_quality's exact= (default: by edge count)")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--host", action="store_true", help="with --time: also the library's host path")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    edges = gr.random_regular_edges(args.n, args.degree, seed=0)
    emb = gr.create_graphem(gr.edges_to_adjacency(args.n, edges), n_components=args.dim, backend="hip", verbose=False,
                            seed=0, init="random", sampler="device")
    exact = None if args.exact is None else args.exact == "yes"
    print("start:", emb.layout_quality(exact=exact, sample_size=args.sample_size))
    emb.run_layout(args.iters)
    print(f"after {args.iters} iterations:", emb.layout_quality(exact=exact, sample_size=args.sample_size))
    if not args.time:
        return
    engine, E = emb._engine, emb.n_edges   # pylint: disable=protected-access
    q = _native.LayoutQuality(emb._edges_np, emb.n, emb.device.index)   # pylint: disable=protected-access
    q.set_positions_device(engine.positions_unpadded_device_ptr(), engine.D)
    rows = np.sort(np.random.default_rng(0).choice(E, min(args.sample_size, E), replace=False))
    q.crossings(rows)   # warm-up: the code object is loaded
    (_, sample_sum), t_est, est_all = timed(lambda: q.crossings(rows), max(args.repeats, 5))
    (_, total), t_exact, exact_all = timed(q.crossings, args.repeats)
    _, t_set, _ = timed(lambda: q.set_positions_device(engine.positions_unpadded_device_ptr(), engine.D), args.repeats)
    _, t_len, _ = timed(q.edge_lengths, args.repeats)
    rec = {"n": args.n, "E": E, "crossings": total // 2, "exact_s": t_exact, "exact_all_s": exact_all,
           "pair_tests_per_s": E * E / t_exact, "estimate_rows": len(rows), "estimate_s": t_est, "estimate_all_s": est_all,
           "estimate": E / (2 * len(rows)) * sample_sum, "set_positions_s": t_set, "edge_lengths_s": t_len}
    q.close()
    if args.host:
        h = _native.LayoutQuality(emb._edges_np, emb.n, -1)   # pylint: disable=protected-access
        h.set_positions(emb.get_positions())
        (_, host_total), t_host, _ = timed(h.crossings, 1)
        h.close()
        assert host_total == total, "host path and device disagree"
        rec.update({"host_exact_s": t_host, "host_threads": min(16, os.cpu_count() or 1)})
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
