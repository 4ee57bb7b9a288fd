"""Graph statistics timings on the GPU (graphem-rapids_amd/graphstats.py, csrc/graphstats.hip): one JSON line per size.

    python tools/graphstats_timing.py [--sizes 20000 100000] [--m 3] [--out profiles/graphstats/timing.jsonl]

On a Barabasi-Albert graph (barabasi_albert_edges, m edges per new vertex) of each size:
  distances_s       CentralityGraph.distances() over every vertex: the bit-parallel pass (24 n bytes per 64 sources);
  closeness_s       CentralityGraph.closeness() on the same graph: the only all-sources distance pass there was before,
                    through the Brandes state of gh_cent_paths (n (32 * 64 + 32) bytes per 64 sources);
  components_s      component_labels(), next to scipy.sparse.csgraph.connected_components on the host;
  triangles_s       triangle_counts(), next to networkx.triangles on the host (sizes up to --nx-max only).
Times are wall-clock around blocking calls (each ends in a device synchronise), the best of --repeat after one warm-up
call of each kind on the same graph.  The two distance passes must agree on reached and dist_sum, or the run fails."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import graphem_rapids_amd as gr  # noqa: E402


def timed(fn, repeat):
    fn()   # warm-up: code objects, allocations of this shape
    best, out = None, None
    for _ in range(repeat):
        t = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t
        best = dt if best is None else min(best, dt)
    return out, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[20_000, 100_000])
    ap.add_argument("--m", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--nx-max", type=int, default=100_000, help="largest size networkx.triangles is timed at")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for n in args.sizes:
        edges = gr.barabasi_albert_edges(n, args.m, seed=1)
        g = gr.CentralityGraph(edges, n=n)
        (reached, dist_sum, ecc), t_dist = timed(g.distances, args.repeat)
        (_, _, reached_b, dist_sum_b), t_close = timed(lambda: g.raw_paths(np.arange(n), False, False, True), args.repeat)
        if not (np.array_equal(reached, reached_b) and np.array_equal(dist_sum, dist_sum_b)):
            raise SystemExit(f"n = {n}: the two distance passes disagree")
        labels, t_comp = timed(g.component_labels, args.repeat)
        tri, t_tri = timed(g.triangle_counts, args.repeat)
        g.close()
        rec = {"graph": "barabasi_albert", "n": n, "m": args.m, "edges": len(edges), "max_degree": int(np.bincount(edges.ravel()).max()),
               "diameter": int(ecc.max()), "distances_s": round(t_dist, 5), "closeness_s": round(t_close, 5),
               "closeness_over_distances": round(t_close / t_dist, 2), "components_s": round(t_comp, 5),
               "triangles_s": round(t_tri, 5), "triangles_total": int(tri.sum()) // 3}
        from scipy.sparse.csgraph import connected_components
        adjacency = gr.edges_to_adjacency(n, edges)
        t = time.perf_counter()
        count, host_labels = connected_components(adjacency, directed=False)
        rec["scipy_components_s"] = round(time.perf_counter() - t, 5)
        if count != len(np.unique(labels)):
            raise SystemExit(f"n = {n}: component counts differ")
        if n <= args.nx_max:
            import networkx as nx
            G = nx.from_scipy_sparse_array(adjacency)
            t = time.perf_counter()
            want = nx.triangles(G)
            rec["networkx_triangles_s"] = round(time.perf_counter() - t, 4)
            if [want[v] for v in range(n)] != tri.tolist():
                raise SystemExit(f"n = {n}: triangle counts differ from networkx")
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
