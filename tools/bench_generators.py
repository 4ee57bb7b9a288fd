"""Times the graph generators against the reference's calls (the networkx function + nx.adjacency_matrix) on the same box.

One warm-up call per shape, then the median of 5 calls; each of ours ends with the download of the edges (and the CSR
build for the generate_* form), which a caller pays and which synchronises.  Prints one JSON line per row and, first, the
cost of creating and destroying an empty generator handle.  Needs a GPU: timing the host path instead would say nothing
about the kernels.

    python tools/bench_generators.py                     every row
    python tools/bench_generators.py --only ba_1m --calls 1 --no-baseline      one family, e.g. under a profiler
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import graphem_rapids_amd as gr  # noqa: E402
from graphem_rapids_amd import _native  # noqa: E402


def big_sbm():
    sizes = 2000 + 80 * np.arange(50)
    sizes[-1] += 200_000 - sizes.sum()
    rng = np.random.default_rng(5)
    P = rng.uniform(2e-5, 8e-5, size=(50, 50))
    P = (P + P.T) / 2
    np.fill_diagonal(P, rng.uniform(2e-3, 8e-3, size=50))
    return sizes.tolist(), P


def rows():
    import networkx as nx

    def adj(G):
        return nx.adjacency_matrix(G, dtype=int)

    def nx_road(w, h):
        G = nx.grid_2d_graph(w, h)
        return adj(nx.relabel_nodes(G, {node: i for i, node in enumerate(G.nodes())}))

    def nx_scale_free(n):
        G = nx.scale_free_graph(n, seed=0).to_undirected()
        G.remove_edges_from(nx.selfloop_edges(G))
        return adj(G)

    sizes, P = big_sbm()
    # name, tier, ours (adjacency), ours (edges only) or None, the reference's call, vertices
    return [
        ("sbm_default", 1, gr.generate_sbm, None, lambda: adj(nx.stochastic_block_model([75] * 4, (np.full((4, 4), 0.01) + np.eye(4) * 0.14), seed=0)), 300),
        ("ba_default", 1, gr.generate_ba, None, lambda: adj(nx.barabasi_albert_graph(300, 3, seed=0)), 300),
        ("geometric_default", 1, gr.generate_geometric, None, lambda: adj(nx.random_geometric_graph(100, 0.2, dim=2, seed=0)), 100),
        ("bipartite_default", 1, lambda: gr.generate_bipartite_graph(seed=0), None, lambda: adj(nx.bipartite.random_graph(50, 100, 0.1, seed=0)), 150),
        ("ws_default", 2, gr.generate_ws, None, lambda: adj(nx.watts_strogatz_graph(1000, 6, 0.3, seed=0)), 1000),
        ("power_cluster_default", 2, gr.generate_power_cluster, None, lambda: adj(nx.powerlaw_cluster_graph(1000, 3, 0.5, seed=0)), 1000),
        ("scale_free_default", 2, gr.generate_scale_free, None, lambda: nx_scale_free(100), 100),
        ("relaxed_caveman_default", 2, gr.generate_relaxed_caveman, None, lambda: adj(nx.relaxed_caveman_graph(10, 10, 0.1, seed=0)), 100),
        ("caveman_default", 2, gr.generate_caveman, None, lambda: adj(nx.caveman_graph(10, 10)), 100),
        ("road_network_default", 2, gr.generate_road_network, None, lambda: nx_road(30, 30), 900),
        ("balanced_tree_default", 2, gr.generate_balanced_tree, None, lambda: adj(nx.balanced_tree(2, 10)), 2047),
        ("sbm_20k", 1, lambda: gr.edges_to_adjacency(20_000, gr.sbm_edges([s // 10 for s in sizes], P * 10, 0)),
         lambda: gr.sbm_edges([s // 10 for s in sizes], P * 10, 0),
         lambda: adj(nx.stochastic_block_model([s // 10 for s in sizes], P * 10, seed=0)), 20_000),
        ("geometric_50k_d2", 1, lambda: gr.generate_geometric(50_000, 0.00798, 2, 0), lambda: gr.geometric_edges(50_000, 0.00798, 2, 0),
         lambda: adj(nx.random_geometric_graph(50_000, 0.00798, dim=2, seed=0)), 50_000),
        ("ba_100k", 1, lambda: gr.generate_ba(100_000, 4, 0), lambda: gr.barabasi_albert_edges(100_000, 4, 0),
         lambda: adj(nx.barabasi_albert_graph(100_000, 4, seed=0)), 100_000),
        ("sbm_200k", 1, lambda: gr.edges_to_adjacency(200_000, gr.sbm_edges(sizes, P, 0)), lambda: gr.sbm_edges(sizes, P, 0),
         lambda: adj(nx.stochastic_block_model(sizes, P, seed=0)), 200_000),
        ("geometric_500k_d2", 1, lambda: gr.generate_geometric(500_000, 0.002523, 2, 0), lambda: gr.geometric_edges(500_000, 0.002523, 2, 0),
         lambda: adj(nx.random_geometric_graph(500_000, 0.002523, dim=2, seed=0)), 500_000),
        ("geometric_500k_d3", 1, lambda: gr.generate_geometric(500_000, 0.01684, 3, 0), lambda: gr.geometric_edges(500_000, 0.01684, 3, 0),
         lambda: adj(nx.random_geometric_graph(500_000, 0.01684, dim=3, seed=0)), 500_000),
        ("ba_1m", 1, lambda: gr.generate_ba(1_000_000, 4, 0), lambda: gr.barabasi_albert_edges(1_000_000, 4, 0),
         lambda: adj(nx.barabasi_albert_graph(1_000_000, 4, seed=0)), 1_000_000),
    ]


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
    ap.add_argument("--only", default=None, help="comma-separated row names")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--baseline-limit", type=float, default=60.0, help="seconds one reference call may take")
    args = ap.parse_args()
    if _native.load().gh_device_count() < 1:
        sys.exit("bench_generators.py needs a GPU")

    def handle():
        _native.Generator(0).close()
    ms = timed(handle, args.calls)
    handle_ms = statistics.median(ms)
    print(json.dumps({"row": "empty_handle_create_destroy", "ms_median": round(handle_ms, 4), "ms": [round(x, 4) for x in ms]}), flush=True)
    only = set(args.only.split(",")) if args.only else None
    last_ratio = {}                          # family -> seconds per vertex of the last reference call, to skip hopeless ones
    for name, tier, ours, ours_edges, theirs, n in rows():
        if only and name not in only:
            continue
        family = name.split("_")[0]
        row = {"row": name, "tier": tier, "vertices": n, "device": bool(tier == 1 and n >= gr.generators.DEVICE_MIN_VERTICES)}
        ms = timed(ours, args.calls)
        row["ours_ms_median"], row["ours_ms"] = round(statistics.median(ms), 4), [round(x, 4) for x in ms]
        if ours_edges is not None:
            ms = timed(ours_edges, args.calls)
            row["ours_edges_ms_median"], row["ours_edges_ms"] = round(statistics.median(ms), 4), [round(x, 4) for x in ms]
        if not args.no_baseline:
            guess = last_ratio.get(family, 0.0) * n
            if guess > args.baseline_limit:
                row["reference_ms_median"] = None
                row["reference_note"] = f"skipped: about {guess:.0f} s by its time at the size before"
            else:
                small = n <= 5000
                t = time.perf_counter()
                ms = timed(theirs, args.calls) if small else []
                if not small:                 # one call, no warm-up: it takes seconds
                    theirs()
                    ms = [(time.perf_counter() - t) * 1e3]
                row["reference_ms_median"], row["reference_ms"] = round(statistics.median(ms), 4), [round(x, 4) for x in ms]
                last_ratio[family] = statistics.median(ms) / 1e3 / n * 1.5
                row["speedup"] = round(row["reference_ms_median"] / row["ours_ms_median"], 2)
                if small:
                    row["within_handle_cost"] = bool(row["ours_ms_median"] <= row["reference_ms_median"] + handle_ms)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
