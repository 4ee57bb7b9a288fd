"""Centrality timings on the GPU (graphem-rapids_amd/centrality.py, csrc/centrality.hip): one JSON line per case.

    python tools/bench_centrality.py [--out profiles/centrality/bench.jsonl] [--quick]

Cases: exact all-sources paths (betweenness + load + closeness in one pass) on random-regular graphs (degree 3) at
10 K and 100 K vertices; sampled paths (k = 1024 sources) at 1 M; PageRank and eigenvector centrality at 1 M (a random 3-regular graph plus Erdos-Renyi edges: connected, not regular); and, for
comparison, networkx's betweenness + load + closeness on the same host at the largest size listed for it (with the GPU
time at that size).  Times are wall-clock around blocking calls, after one warm-up call of each kind.  --quick: the
small sizes only (the run the kernel profile is taken from)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import graphem_rapids_amd as gr  # noqa: E402
from graphem_rapids_amd import centrality as cent  # noqa: E402


def timed(fn, repeat=1):
    best = None
    for _ in range(repeat):
        t = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t
        best = dt if best is None else min(best, dt)
    return out, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "centrality", "bench.jsonl"))
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--nx-n", type=int, default=2000, help="size of the networkx comparison")
    args = ap.parse_args()
    lines = []

    def emit(**rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    warm = cent.CentralityGraph(gr.random_regular_edges(1000, 3, seed=0), n=1000)
    warm.paths()
    warm.pagerank()
    warm.eigenvector()
    warm.close()

    exact_sizes = [10_000] if args.quick else [10_000, 100_000]
    for n in exact_sizes:
        g = cent.CentralityGraph(gr.random_regular_edges(n, 3, seed=1), n=n)
        _, dt = timed(g.paths)
        emit(case="paths_exact", graph="random_regular", n=n, degree=3, sources=n, seconds=round(dt, 4),
             us_per_source=round(1e6 * dt / n, 3))
        g.close()

    if not args.quick:
        n = 1_000_000
        g = cent.CentralityGraph(gr.random_regular_edges(n, 3, seed=2), n=n)
        src = cent.sample_sources(range(n), 1024, 0)
        _, dt = timed(lambda: g.paths(src))
        emit(case="paths_sampled", graph="random_regular", n=n, degree=3, sources=1024, seconds=round(dt, 4),
             us_per_source=round(1e6 * dt / 1024, 3))
        g.close()
        # PageRank and eigenvector on a connected graph that is not regular (on a regular graph the uniform start is
        # already PageRank's answer): a random 3-regular graph plus Erdos-Renyi edges of mean degree 5
        edges = np.concatenate([gr.random_regular_edges(n, 3, seed=3), gr.erdos_renyi_edges(n, 5.0 / n, seed=3)])
        g = cent.CentralityGraph(edges, n=n)
        # networkx's default stop, L1 change < N * tol = 1 at tol = 1e-6, ends after one iteration here; 1e-12 runs on
        for tol in (1e-6, 1e-12):
            (x, its), dt = timed(lambda: g.pagerank(tol=tol, return_iterations=True), repeat=3)
            emit(case="pagerank", graph="rr3+er5", n=n, edges=g._g.edges, tol=tol, iterations=its, seconds=round(dt, 4),
                 ms_per_iteration=round(1e3 * dt / its, 4))
        _, dt = timed(g.eigenvector)
        emit(case="eigenvector", graph="rr3+er5", n=n, edges=g._g.edges, seconds=round(dt, 4))
        g.close()

    try:
        import networkx as nx
    except ImportError:
        nx = None
    if nx is not None:
        n = args.nx_n if not args.quick else 500
        edges = gr.random_regular_edges(n, 3, seed=4)
        G = nx.Graph()
        G.add_nodes_from(range(n))
        G.add_edges_from(edges.tolist())
        t = time.perf_counter()
        nx.betweenness_centrality(G)
        nx.load_centrality(G)
        nx.closeness_centrality(G)
        t_nx = time.perf_counter() - t
        g = cent.CentralityGraph(edges, n=n)
        _, dt = timed(g.paths, repeat=3)
        g.close()
        emit(case="networkx_vs_gpu", graph="random_regular", n=n, degree=3, networkx_seconds=round(t_nx, 3),
             gpu_seconds=round(dt, 5), speedup=round(t_nx / dt, 1))

    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
