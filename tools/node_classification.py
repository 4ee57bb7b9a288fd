"""How well do a layout's nearest labelled neighbours, and label propagation on the graph, recover a stochastic block model's
blocks from a few known labels, and the time the classification kernels take.

    python tools/node_classification.py --blocks 16 --n-per-block 6250 --iters 20 [--host] [--host-rows 2048]

Builds an SBM of --blocks blocks of --n-per-block vertices with mean degrees --deg-in inside and --deg-out outside a block,
runs the layout for --iters iterations, keeps --train-fraction of the labels (split_labels, stratified) and predicts the rest:
knn_classify with --k neighbours on the embedder's device positions, label_propagation on the graph, and the majority class.
Times are host clocks around blocking calls (every call ends in a stream synchronise), after one warm-up call, the minimum of
--repeats: gh_qual_knn_vote over the test rows (a pair is one (row, training row): pairs per second = rows * T / time), with
--host also the library's host path on the first --host-rows test rows, whose output must equal the device's, and
gh_cent_label_propagation on a handle that is already built.  One JSON line at the end.
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
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--n-per-block", type=int, default=6250)
    ap.add_argument("--deg-in", type=float, default=8.0)
    ap.add_argument("--deg-out", type=float, default=1.0)
    ap.add_argument("--dim", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--train-fraction", type=float, default=0.1)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--host", action="store_true", help="also the library's host path")
    ap.add_argument("--host-rows", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    B, m = args.blocks, args.n_per_block
    n = B * m
    P = np.full((B, B), args.deg_out / max(n - m, 1))
    np.fill_diagonal(P, args.deg_in / max(m - 1, 1))
    edges = gr.sbm_edges([m] * B, P, seed=0)
    planted = np.repeat(np.arange(B), m)
    emb = gr.create_graphem(gr.edges_to_adjacency(n, edges), n_components=args.dim, backend="hip", verbose=False, seed=0, init="random",
                            sampler="device")
    emb.run_layout(args.iters)
    split = gr.split_labels(planted, args.train_fraction, seed=0)
    train, test = split["train"], split["test"]
    truth = planted[test]
    T, R = len(train), len(test)
    rec = {"n": n, "D": args.dim, "edges": int(len(edges)), "iters": args.iters, "k": args.k, "n_train": T, "n_test": R}

    def score(name, pred):
        rec[name] = {"accuracy": gr.accuracy(truth, pred), "macro_f1": gr.macro_f1(truth, pred)}
        print(f"{name}:", rec[name])

    score("embedding_knn", gr.knn_classify(emb, train, planted[train], k=args.k, rows=test)["pred"])
    seeds = np.full(n, -1)
    seeds[train] = planted[train]
    g = gr.CentralityGraph(edges, n=n)
    spread = gr.label_propagation(g, seeds)
    rec.update({"propagation_rounds": spread["rounds"], "propagation_converged": spread["converged"],
                "propagation_unreached": int((spread["labels"][test] < 0).sum())})
    score("label_propagation", spread["labels"][test])
    score("majority", np.full(R, np.bincount(planted[train]).argmax()))

    engine = emb._engine   # pylint: disable=protected-access
    no_edges = np.zeros((0, 2), dtype=np.int32)
    q = _native.LayoutQuality(no_edges, n, emb.device.index)
    q.set_positions_device(engine.positions_unpadded_device_ptr(), engine.D)
    labels = planted[train].astype(np.int32)
    dev = q.knn_vote(args.k, train, labels, test)   # warm-up
    _, t_knn, knn_all = timed(lambda: q.knn_vote(args.k, train, labels, test), args.repeats)
    rec.update({"knn_s": t_knn, "knn_all_s": knn_all, "knn_pairs_per_s": R * T / t_knn})
    q.close()
    g._g.label_propagation(seeds, B)   # pylint: disable=protected-access
    _, t_lp, lp_all = timed(lambda: g._g.label_propagation(seeds, B), args.repeats)   # pylint: disable=protected-access
    rec.update({"propagation_s": t_lp, "propagation_all_s": lp_all, "propagation_round_s": t_lp / max(spread["rounds"], 1)})
    g.close()
    if args.host:
        few = test[:args.host_rows]
        h = _native.LayoutQuality(no_edges, n, -1)
        h.set_positions(emb.get_positions().astype(np.float32))
        host, t_host, _ = timed(lambda: h.knn_vote(args.k, train, labels, few), 1)
        h.close()
        for a, b in zip(host, dev):
            assert a.tobytes() == b[:len(few)].tobytes(), "host path and device disagree"
        rec.update({"host_rows": len(few), "host_knn_s": t_host, "host_pairs_per_s": len(few) * T / t_host,
                    "host_threads": min(16, os.cpu_count() or 1)})
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
