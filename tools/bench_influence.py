"""Independent Cascade benchmark (csrc/influence.hip): one JSON line per case.

    python tools/bench_influence.py [--repeat 5] [--cases spread_p01,spread_p02,greedy_10k,greedy_100k,ris_100k,ris_1m]

Every graph is random-regular (degree d), so a cascade evaluates exactly d coins per reached (vertex, trial) and the coin
count of a call is d * (sum of the spreads of every breadth-first search it ran).  Reported per case: ms per call (median
of --repeat after one warm-up call), coins per second, and that rate over the VALU bound for one mix per coin:
VALU_PER_COIN vector instructions per coin (counted in the gfx950 ISA of the push loop, integer multiplies at the full
rate) at 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz.  numpy_est_ms: the same coin count at the rate numpy computes
tests/ic_reference.py's mix (measured in the run); the restatement itself is far slower than that floor at these sizes.

ris_100k / ris_1m (not in the default list): reverse influence sampling at p = 0.1 with theta = 2^20 sets -- ms to draw the
collection, its members and members per second, ms of maximum coverage for k = 10 and 50 -- and the epsilon mode at
epsilon = 0.1 (at most --ris-max-samples sets per collection).  Every seed set, CELF's at 100 K included, is then scored by
one common evaluation: g.spread over 4096 trials with a seed none of the selections used, mean and standard error.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import graphem_rapids_amd as gr  # noqa: E402
from graphem_rapids_amd.influence import InfluenceGraph, celf_greedy, ris_seed_selection  # noqa: E402
import ic_reference as ref  # noqa: E402

VALU_PER_COIN = 20
LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9
DEG = 8


def numpy_coin_rate():
    z = np.arange(1 << 22, dtype=np.uint64)
    t0 = time.perf_counter()
    ref.mix(ref.mix(z) ^ z)   # one coin = two mixes of an array, the restatement's inner step
    return len(z) / (time.perf_counter() - t0)


def timed(fn, repeat):
    fn()
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, out


def spread_case(name, g, p, T, repeat, np_rate):
    seeds = np.random.default_rng(1).choice(g.n, 10, replace=False)
    ms, (mean, trials) = timed(lambda: g.spread(seeds, p, T, None, 7, return_trials=True), repeat)
    coins = DEG * int(trials.sum(dtype=np.int64))
    return dict(case=name, n=g.n, p=p, trials=T, seeds=10, ms=round(ms, 3), mean_spread=mean, coins=coins)


def greedy_case(name, g, p, T, k, repeat, np_rate):
    calls = []

    def evaluate(base, cand):
        tot = g.marginal_totals(base, cand, p, T, None, 7)
        calls.append((tuple(base), len(cand), int(tot.sum())))
        return tot
    ms, (seeds, evals) = timed(lambda: celf_greedy(evaluate, g.n, k), repeat)
    calls = calls[len(calls) // (repeat + 1) * repeat:]   # the last call's evaluations
    base_tot = {}
    coins = 0
    for base, ncand, marg in calls:
        if base not in base_tot:
            base_tot[base] = int(g.spread(list(base), p, T, None, 7, return_trials=True)[1].sum()) if base else 0
        coins += DEG * (marg + (ncand + (1 if base else 0)) * base_tot[base])
    return dict(case=name, n=g.n, p=p, trials=T, k=k, ms=round(ms, 3), seeds_chosen=seeds, evaluations=evals, coins=coins)


def common_spread(g, seeds, p):
    """(mean, standard error) of the spread under the evaluation every selection shares."""
    _, trials = g.spread(seeds, p, 4096, None, 12345, return_trials=True)
    return round(float(trials.mean()), 3), round(float(trials.std(ddof=1) / np.sqrt(len(trials))), 3)


def ris_case(name, n, max_samples):
    p, theta = 0.1, 1 << 20
    g = InfluenceGraph(gr.random_regular_edges(n, DEG, seed=1), n=n)
    g.rr_sets(64, p, None, 7).close()   # warm-up: the chunk state is allocated once
    t0 = time.perf_counter()
    coll = g.rr_sets(theta, p, None, 7)
    sample_ms = (time.perf_counter() - t0) * 1e3
    members = coll.n_members
    r = dict(case=name, n=n, p=p, samples=theta, sample_ms=round(sample_ms, 3), members=members,
             members_per_s=float(f"{members / (sample_ms * 1e-3):.4g}"))
    for k in (10, 50):
        coll.cover(k)
        t0 = time.perf_counter()
        seeds, gains = coll.cover(k)
        r[f"cover_k{k}_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        r[f"estimate_k{k}"] = round(n * int(gains.sum()) / theta, 3)
        r[f"spread_k{k}"], r[f"spread_k{k}_se"] = common_spread(g, seeds, p)
    coll.close()
    t0 = time.perf_counter()
    seeds, info = ris_seed_selection(g, 10, p, epsilon=0.1, max_samples=max_samples, seed=7)
    r.update(eps_ms=round((time.perf_counter() - t0) * 1e3, 3), eps_samples=info["samples"], eps_rounds=info["rounds"],
             eps_ratio=round(info["ratio"], 4), eps_lower=round(info["lower"], 3), eps_upper=round(info["upper"], 3))
    r["eps_spread_k10"], r["eps_spread_k10_se"] = common_spread(g, seeds, p)
    if n <= 100_000:   # CELF over Monte Carlo, the baseline this replaces at sizes it cannot reach
        t0 = time.perf_counter()
        seeds, evals = g.greedy(10, p, 256, None, 7)
        r.update(greedy_ms=round((time.perf_counter() - t0) * 1e3, 3), greedy_evaluations=evals)
        r["greedy_spread_k10"], r["greedy_spread_k10_se"] = common_spread(g, seeds, p)
    g.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ris-max-samples", type=int, default=1 << 22)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--cases", default="spread_p01,spread_p02,greedy_10k,greedy_100k")
    args = ap.parse_args()
    if gr._native.device_count() < 1:
        raise SystemExit("no GPU visible: this tool measures the MI355X")
    np_rate = numpy_coin_rate()
    cases = args.cases.split(",")
    rr1m = None
    for c in cases:
        if c.startswith("ris"):
            print(json.dumps(ris_case(c, 100_000 if c == "ris_100k" else 1 << 20, args.ris_max_samples)), flush=True)
            continue
        if c.startswith("spread"):
            if rr1m is None:
                rr1m = InfluenceGraph(gr.random_regular_edges(1 << 20, DEG, seed=0), n=1 << 20)
            r = spread_case(c, rr1m, 0.1 if c == "spread_p01" else 0.2, 1024, args.repeat, np_rate)
        else:
            n = 10_000 if c == "greedy_10k" else 100_000
            g = InfluenceGraph(gr.random_regular_edges(n, DEG, seed=1), n=n)
            r = greedy_case(c, g, 0.1, 256, 10, max(1, args.repeat // 2), np_rate)
            g.close()
        rate = r["coins"] / (r["ms"] * 1e-3)
        r.update(coins_per_s=float(f"{rate:.4g}"), valu_bound_coins_per_s=float(f"{LANE_OPS_PER_S / VALU_PER_COIN:.4g}"),
                 share_of_valu_bound=round(rate / (LANE_OPS_PER_S / VALU_PER_COIN), 4),
                 numpy_est_ms=round(r["coins"] / np_rate * 1e3, 1))
        r["speedup_vs_numpy_est"] = round(r["numpy_est_ms"] / r["ms"], 1)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
