"""Link-score timings on the GPU (graphem-rapids_amd/links.py, csrc/links.hip): one JSON line.

    python tools/bench_links.py [--n 100000] [--m 5] [--pairs 1000000] [--k 10] [--nx-pairs 10000] [--out FILE]

On barabasi_albert_edges(n, m):
  link_scores_s        CentralityGraph.link_scores over --pairs random vertex pairs (cn, aa and ra of each);
  candidates_s         CentralityGraph.link_candidates(score, k) over every vertex, for each of the five scores;
  hub_source_s         the same call for the largest-degree vertex alone: one workgroup serves it, so this is the floor of
                       candidates_s, and hub_share = hub_source_s / candidates_s says how much of the whole call it is;
  top_sources_s, low_sources_s   the 1024 largest-degree and the 1024 smallest-degree sources, for the spread between them;
  slabs                workgroups (each with a slab) the all-vertex call runs at the default budget: min(1024, n,
                       1 GiB / 20 n);
  networkx_s           networkx.adamic_adar_index + resource_allocation_index + jaccard_coefficient over the first
                       --nx-pairs of the same pairs, on the host, next to link_scores_subsample_s for the same pairs here.
Times are wall-clock around blocking calls (each ends in a device synchronise), the best of --repeat after one warm-up
call of each kind.  The subsample's scores must agree with networkx within (common neighbours) * 2^-32, or the run fails."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import graphem_rapids_amd as gr  # noqa: E402
from graphem_rapids_amd import links  # noqa: E402


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
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--m", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nx-pairs", type=int, default=10_000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.n
    edges = gr.barabasi_albert_edges(n, args.m, seed=1)
    g = gr.CentralityGraph(edges, n=n)
    deg = g.degree()
    by_degree = np.argsort(-deg, kind="stable")
    pairs = np.random.default_rng(0).integers(0, n, size=(args.pairs, 2))
    rec = {"graph": "barabasi_albert", "n": n, "m": args.m, "edges": len(g.edges), "max_degree": int(deg.max()),
           "pairs": args.pairs, "k": args.k, "slabs": int(min(1024, n, (1 << 30) // (20 * n)))}

    (cn, _, _), t = timed(lambda: g.link_scores(pairs), args.repeat)
    rec["link_scores_s"] = round(t, 5)
    rec["pairs_with_common_neighbours"] = int((cn > 0).sum())
    everyone = np.arange(n)
    for score in links.LINK_SCORES:
        (ids, _, _), t = timed(lambda s=score: g.link_candidates(s, args.k, everyone), args.repeat)
        rec[f"candidates_{score}_s"] = round(t, 5)
        if score == "adamic_adar":
            rec["sources_with_k_candidates"] = int((ids[:, -1] >= 0).sum())
            _, hub = timed(lambda: g.link_candidates("adamic_adar", args.k, by_degree[:1]), args.repeat)
            _, top = timed(lambda: g.link_candidates("adamic_adar", args.k, by_degree[:1024]), args.repeat)
            _, low = timed(lambda: g.link_candidates("adamic_adar", args.k, by_degree[-1024:]), args.repeat)
            rec.update({"hub_source_s": round(hub, 5), "hub_share": round(hub / t, 3), "top_sources_s": round(top, 5),
                        "low_sources_s": round(low, 5)})

    sub = pairs[: args.nx_pairs]
    sub = sub[sub[:, 0] != sub[:, 1]]
    ours, t = timed(lambda: links._scores(g, sub), args.repeat)   # pylint: disable=protected-access
    rec["link_scores_subsample_s"] = round(t, 5)
    g.close()
    import networkx as nx
    G = nx.empty_graph(n)
    G.add_edges_from(edges.tolist())
    ebunch = [tuple(p) for p in sub.tolist()]
    t = time.perf_counter()
    theirs = {"adamic_adar": [p for _, _, p in nx.adamic_adar_index(G, ebunch)],
              "resource_allocation": [p for _, _, p in nx.resource_allocation_index(G, ebunch)],
              "jaccard": [p for _, _, p in nx.jaccard_coefficient(G, ebunch)]}
    rec["networkx_s"] = round(time.perf_counter() - t, 4)
    rec["networkx_pairs"] = len(ebunch)
    bound = np.maximum(ours["common_neighbors"], 0) * 2.0 ** -32
    for key in ("adamic_adar", "resource_allocation"):
        if not (np.abs(ours[key] - np.array(theirs[key])) <= bound).all():
            raise SystemExit(f"{key} differs from networkx beyond its bound")
    if ours["jaccard"].tolist() != [float(p) for p in theirs["jaccard"]]:
        raise SystemExit("jaccard differs from networkx")
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as fh:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
