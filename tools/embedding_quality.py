"""Embedding quality of a generated graph before and after run_layout, and the time the neighbour ranks take.

    python tools/embedding_quality.py --n 100000 --iters 20 --time [--host] [--graph ba]

Prints embedding_quality() of a random-regular graph's start (--graph ba: a Barabasi-Albert graph with m = --degree / 2,
the hub-heavy case) and of its layout after --iters iterations.  --time measures, on the final layout, neighbor_ranks over
all sources (skipped with --no-all) and over --sample-size sampled sources, and with --host the library's host path on the
sampled sources.  Times are host clocks around blocking calls (every call ends in a stream synchronise), after one warm-up
call, the minimum of --repeats; a pair is one (source, column): pairs per second = sources * n / time.  One JSON line at
the end.
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
    ap.add_argument("--graph", default="rr", choices=["rr", "ba"])
    ap.add_argument("--sample-size", type=int, default=4096)
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--no-all", action="store_true", help="with --time: skip the all-sources call")
    ap.add_argument("--host", action="store_true", help="with --time: also the library's host path, on the sampled sources")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    n = args.n
    if args.graph == "rr":
        edges = gr.random_regular_edges(n, args.degree, seed=0)
    else:
        edges = gr.barabasi_albert_edges(n, args.degree // 2, seed=0)
    emb = gr.create_graphem(gr.edges_to_adjacency(n, edges), n_components=args.dim, backend="hip", verbose=False,
                            seed=0, init="random", sampler="device")
    print("start:", emb.embedding_quality(exact=False, sample_size=args.sample_size))
    emb.run_layout(args.iters)
    print(f"after {args.iters} iterations:", emb.embedding_quality(exact=False, sample_size=args.sample_size))
    if not args.time:
        return
    engine = emb._engine   # pylint: disable=protected-access
    q = _native.LayoutQuality(emb._edges_np, n, emb.device.index)   # pylint: disable=protected-access
    q.set_positions_device(engine.positions_unpadded_device_ptr(), engine.D)
    rows = np.sort(np.random.default_rng(0).choice(n, min(args.sample_size, n), replace=False))
    sampled = q.neighbor_ranks(rows)   # warm-up: the code object is loaded, the graph is built
    _, t_sample, sample_all = timed(lambda: q.neighbor_ranks(rows), max(args.repeats, 5))
    rec = {"graph": args.graph, "n": n, "D": args.dim, "iters": args.iters, "max_degree": int(np.bincount(emb._edges_np.ravel()).max()),   # pylint: disable=protected-access
           "sample_sources": len(rows), "sample_slots": len(sampled[1]), "sample_s": t_sample, "sample_all_s": sample_all,
           "sample_pairs_per_s": len(rows) * n / t_sample}
    if not args.no_all:
        full, t_all, all_all = timed(q.neighbor_ranks, args.repeats)
        rec.update({"all_slots": len(full[1]), "all_s": t_all, "all_all_s": all_all, "all_pairs_per_s": n * n / t_all})
        _, t_whole, _ = timed(lambda: emb.embedding_quality(exact=True), 1)
        rec["embedding_quality_exact_s"] = t_whole
    q.close()
    if args.host:
        h = _native.LayoutQuality(emb._edges_np, n, -1)   # pylint: disable=protected-access
        h.set_positions(emb.get_positions().astype(np.float32))
        h.neighbor_ranks(rows[:16])
        host, t_host, _ = timed(lambda: h.neighbor_ranks(rows), 1)
        h.close()
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(host, sampled)), "host path and device disagree"
        rec.update({"host_sample_s": t_host, "host_pairs_per_s": len(rows) * n / t_host, "host_threads": min(16, os.cpu_count() or 1)})
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
