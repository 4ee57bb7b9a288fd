"""Do the k-means clusters of a layout recover a stochastic block model's blocks, and the time the clustering kernels take.

    python tools/cluster_quality.py --blocks 16 --n-per-block 6250 --iters 20 --time [--host] [--all]

Builds an SBM of --blocks blocks of --n-per-block vertices with mean degrees --deg-in inside and --deg-out outside a block,
runs the layout for --iters iterations and prints cluster_recovery() of it against the planted blocks and, unless
--no-louvain, against the Louvain communities of the graph.  --time measures, on the final layout: one Lloyd iteration (the
difference of two gh_qual_kmeans calls with 1 and 1 + --lloyd-iters updates from the same random start, divided by the
updates the second ran beyond the first), the k-means++ seed steps, and the silhouette's distance sums over --sample-size
sampled rows; with --all also over all n rows; with --host the library's host path on the same inputs (the sums on
--host-rows of the sampled rows).  Times are host clocks around blocking calls (every call ends in a stream synchronise),
after one warm-up call, the minimum of --repeats; a pair is one (row, column): pairs per second = rows * n / time.  One JSON
line at the end.
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


def lloyd_time(q, start, iters, repeats):
    """(seconds per Lloyd iteration, updates measured, the longer run)."""
    q.kmeans(start, 1)   # warm-up
    one, t_one, _ = timed(lambda: q.kmeans(start, 1), repeats)
    many, t_many, _ = timed(lambda: q.kmeans(start, 1 + iters), repeats)
    extra = many["n_iter"] - one["n_iter"]
    return ((t_many - t_one) / extra if extra > 0 else float("nan")), extra, many


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--n-per-block", type=int, default=6250)
    ap.add_argument("--deg-in", type=float, default=8.0)
    ap.add_argument("--deg-out", type=float, default=1.0)
    ap.add_argument("--dim", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--n-init", type=int, default=4)
    ap.add_argument("--sample-size", type=int, default=4096)
    ap.add_argument("--no-louvain", action="store_true")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--lloyd-iters", type=int, default=10)
    ap.add_argument("--all", action="store_true", help="with --time: also the distance sums over all n rows on the device")
    ap.add_argument("--host", action="store_true", help="with --time: also the library's host path")
    ap.add_argument("--host-rows", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    B, m = args.blocks, args.n_per_block
    n, k = B * m, B
    P = np.full((B, B), args.deg_out / max(n - m, 1))
    np.fill_diagonal(P, args.deg_in / max(m - 1, 1))
    edges = gr.sbm_edges([m] * B, P, seed=0)
    planted = np.repeat(np.arange(B), m)
    adjacency = gr.edges_to_adjacency(n, edges)
    emb = gr.create_graphem(adjacency, n_components=args.dim, backend="hip", verbose=False, seed=0, init="random", sampler="device")
    emb.run_layout(args.iters)

    def show(name, truth):
        r = gr.cluster_recovery(emb, truth, k=k, n_init=args.n_init, sample_size=args.sample_size)
        r.pop("labels")
        print(f"{name}:", r)
        return r
    rec = {"n": n, "D": args.dim, "k": k, "edges": int(len(edges)), "iters": args.iters, "planted": show("against the planted blocks", planted)}
    if not args.no_louvain:
        found = gr.community_labels(adjacency)
        rec["louvain_communities"] = int(len(np.unique(found)))
        rec["louvain"] = show("against the Louvain communities", found)
        rec["louvain_vs_planted_ari"] = gr.adjusted_rand_index(found, planted)
    if not args.time:
        print(json.dumps(rec))
        return
    engine = emb._engine   # pylint: disable=protected-access
    no_edges = np.zeros((0, 2), dtype=np.int32)
    q = _native.LayoutQuality(no_edges, n, emb.device.index)
    q.set_positions_device(engine.positions_unpadded_device_ptr(), engine.D)
    start = q.position_rows(np.sort(np.random.default_rng(0).choice(n, k, replace=False)))
    per_iter, extra, run = lloyd_time(q, start, args.lloyd_iters, args.repeats)
    labels = run["labels"]
    bytes_per_iter = n * (4 * args.dim + 12)   # the rows and the previous labels read, the labels and d2 written
    rec.update({"lloyd_iter_s": per_iter, "lloyd_updates_timed": extra, "lloyd_bytes": bytes_per_iter,
                "lloyd_bytes_per_s": bytes_per_iter / per_iter})
    q.kmeans_seed_step(0, True)
    _, t_seed, _ = timed(lambda: q.kmeans_seed_step(1, False), max(args.repeats, 5))
    rec["seed_step_s"] = t_seed
    _, t_pp, _ = timed(lambda: gr.kmeans_plusplus(emb, k), args.repeats)
    rec["kmeans_plusplus_s"] = t_pp
    rows = np.sort(np.random.default_rng(0).choice(n, min(args.sample_size, n), replace=False))
    sampled = q.cluster_distance_sums(labels, k, rows)   # warm-up
    _, t_sample, sample_all = timed(lambda: q.cluster_distance_sums(labels, k, rows), max(args.repeats, 5))
    rec.update({"sample_rows": len(rows), "sample_s": t_sample, "sample_all_s": sample_all, "sample_pairs_per_s": len(rows) * n / t_sample})
    _, t_score, _ = timed(lambda: gr.silhouette_score(emb, labels, exact=False, sample_size=args.sample_size), 1)
    rec["silhouette_score_sampled_s"] = t_score
    if args.all:
        _, t_all, all_all = timed(lambda: q.cluster_distance_sums(labels, k), args.repeats)
        rec.update({"all_s": t_all, "all_all_s": all_all, "all_pairs_per_s": n * n / t_all})
    q.close()
    if args.host:
        h = _native.LayoutQuality(no_edges, n, -1)
        h.set_positions(emb.get_positions().astype(np.float32))
        host_run, t_one, _ = timed(lambda: h.kmeans(start, 1), 1)
        host_many, t_many, _ = timed(lambda: h.kmeans(start, 1 + args.lloyd_iters), 1)
        for key in ("labels", "d2", "centers", "counts"):
            assert host_many[key].tobytes() == run[key].tobytes(), f"host path and device disagree on {key}"
        extra_h = host_many["n_iter"] - host_run["n_iter"]
        few = rows[:args.host_rows]
        host_sums, t_host, _ = timed(lambda: h.cluster_distance_sums(labels, k, few), 1)
        h.close()
        assert np.allclose(host_sums, sampled[:len(few)], rtol=1e-9, atol=0.0), "host path and device disagree on the sums"
        rec.update({"host_lloyd_iter_s": (t_many - t_one) / extra_h if extra_h > 0 else float("nan"), "host_rows": len(few),
                    "host_sums_s": t_host, "host_pairs_per_s": len(few) * n / t_host, "host_threads": min(16, os.cpu_count() or 1)})
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
