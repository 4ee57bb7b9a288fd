"""Distance preservation of a generated graph before and after run_layout, and the time the hop profile takes.

    python tools/distance_quality.py --n 100000 --iters 20 --time [--host] [--all]

Prints distance_quality() of a random-regular graph's start and of its layout after --iters iterations, from --sample-size
sampled sources.  --time measures, on the final layout, the hop profile over the sampled sources on the device, with --all
also over all n sources, and with --host the library's host path on the sampled sources.  Times are host clocks around
blocking calls (every call ends in a stream synchronise), after one warm-up call, the minimum of --repeats; a pair is one
(source, vertex): pairs per second = sum(reach) / time.  One JSON line at the end.
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
    ap.add_argument("--sample-size", type=int, default=1024)
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--all", action="store_true", help="with --time: also all n sources on the device")
    ap.add_argument("--host", action="store_true", help="with --time: also the library's host path, on the sampled sources")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    n = args.n
    edges = gr.random_regular_edges(n, args.degree, seed=0)
    emb = gr.create_graphem(gr.edges_to_adjacency(n, edges), n_components=args.dim, backend="hip", verbose=False,
                            seed=0, init="random", sampler="device")
    print("start:", gr.distance_quality(emb, exact=False, sample_size=args.sample_size))
    emb.run_layout(args.iters)
    print(f"after {args.iters} iterations:", gr.distance_quality(emb, exact=False, sample_size=args.sample_size))
    if not args.time:
        return
    engine = emb._engine   # pylint: disable=protected-access
    q = _native.LayoutQuality(emb._edges_np, n, emb.device.index)   # pylint: disable=protected-access
    q.set_positions_device(engine.positions_unpadded_device_ptr(), engine.D)
    src = np.sort(np.random.default_rng(0).choice(n, min(args.sample_size, n), replace=False))
    sampled = q.hop_profile(src)   # warm-up: the code object is loaded, the graph is built and uploaded
    pairs = int(sampled["reach"].sum())
    _, t_sample, sample_all = timed(lambda: q.hop_profile(src), max(args.repeats, 5))
    rec = {"n": n, "D": args.dim, "degree": args.degree, "iters": args.iters, "sample_sources": len(src), "sample_pairs": pairs,
           "max_hop": len(sampled["pairs"]), "sample_s": t_sample, "sample_all_s": sample_all, "sample_pairs_per_s": pairs / t_sample}
    _, t_whole, _ = timed(lambda: gr.distance_quality(emb, exact=False, sample_size=args.sample_size), 1)
    rec["distance_quality_sampled_s"] = t_whole
    if args.all:
        full, t_all, all_all = timed(q.hop_profile, args.repeats)
        rec.update({"all_pairs": int(full["reach"].sum()), "all_s": t_all, "all_all_s": all_all,
                    "all_pairs_per_s": int(full["reach"].sum()) / t_all})
    q.close()
    if args.host:
        h = _native.LayoutQuality(emb._edges_np, n, -1)   # pylint: disable=protected-access
        h.set_positions(emb.get_positions().astype(np.float32))
        h.hop_profile(src[:16])
        host, t_host, _ = timed(lambda: h.hop_profile(src), 1)
        h.close()
        for key in ("pairs", "reach", "eccentricity", "min_d2", "max_d2"):
            assert host[key].tobytes() == sampled[key].tobytes(), f"host path and device disagree on {key}"
        rec.update({"host_sample_s": t_host, "host_pairs_per_s": pairs / t_host, "host_threads": min(16, os.cpu_count() or 1),
                    "device_over_host": t_host / t_sample})
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
