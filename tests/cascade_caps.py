"""The graphs, seed sets, samples and set system of the shapes A - E of tests/launch_caps.py, and what the numpy restatements
give for them, each computed once per process: tests/test_launch_caps_cpu.py reads the frontier sizes of the levels off the
restatements (so that a shape keeps reaching the second trip of the kernel its row names), and
tests/test_hip_cascade_caps.py compares the kernels with the same results.  Nothing here touches the library under test
but its host-side graph generators."""
import functools

import numpy as np

import graphem_rapids_amd as gr

import arc_ic_reference as arc
import ic_reference as ic
import launch_caps as lc
import ris_reference as ris

IC_SEED = 7


def _out_regular(n_live, degree, rng):
    """(n_live * degree, 2) int64: every vertex u < n_live with `degree` distinct targets v != u, v < n_live."""
    u = np.arange(n_live, dtype=np.int64)
    v = np.sort(rng.integers(0, n_live, size=(n_live, degree)), axis=1)
    while True:   # redraw the few rows with a repeat or a loop until none is left
        bad = (v[:, 1:] == v[:, :-1]).any(axis=1) | (v == u[:, None]).any(axis=1)
        if not bad.any():
            return np.column_stack([np.repeat(u, degree), v.ravel()])
        v[bad] = np.sort(rng.integers(0, n_live, size=(int(bad.sum()), degree)), axis=1)


# ---- A: forward pull, advance, count, reset ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def forward_pull():
    """(n, canonical pairs, seed sets, (A, 2) probabilities): er2000 of tests/test_hip_influence.py and its three isolated
    vertices; the last set, which straddles the trip boundary of the dense state, holds one of them."""
    s = lc.FWD_PULL
    n = s["n"]
    pairs = ic.canonical_arcs(n, gr.erdos_renyi_edges(n - 3, 0.004, seed=1), False)
    rng = np.random.default_rng(17)
    sets = [sorted(rng.choice(n - 3, s["set_size"], replace=False).tolist()) for _ in range(s["sets"])]
    sets[-1][-1] = n - 1
    prob = arc.mixed_probabilities(rng, (len(pairs), 2), s["arc_scale"])
    return n, pairs, sets, prob


@functools.lru_cache(maxsize=None)
def forward_pull_expected(arcs):
    """((sets, T) int64 counts, frontier entries of the chunk per level, touched entries of the chunk)."""
    s = lc.FWD_PULL
    n, pairs, sets, prob = forward_pull()
    rows, fronts = [], []
    for seeds in sets:
        f = ic.Frontiers()
        if arcs:
            rows.append(arc.spread_trials_arcs(n, pairs, False, prob, seeds, s["T"], IC_SEED, None, frontiers=f))
        else:
            rows.append(ic.spread_trials(n, pairs, False, seeds, s["p"], s["T"], IC_SEED, None, frontiers=f))
        fronts.append(f)
    depth = max(len(f.entries()) for f in fronts)
    entries = [sum(f.entries()[r] for f in fronts if r < len(f.entries())) for r in range(depth)]
    return np.array(rows), entries, sum(f.touched_entries() for f in fronts)


# ---- B: forward push -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def forward_push():
    """(n, canonical pairs, seed sets, (A,) probabilities): out-degree 3 on all but the three isolated vertices, one of
    which is a seed of the last set."""
    s = lc.FWD_PUSH
    n = s["n"]
    rng = np.random.default_rng(23)
    pairs = ic.canonical_arcs(n, _out_regular(n - 3, s["out_degree"], rng), True)
    sets = [np.sort(rng.choice(n - 3, s["set_size"], replace=False)) for _ in range(s["sets"])]
    sets[-1][-1] = n - 1
    prob = arc.mixed_probabilities(rng, len(pairs), s["arc_scale"])
    return n, pairs, sets, prob


@functools.lru_cache(maxsize=None)
def forward_push_expected(arcs):
    """(sets, T) int64 counts after one hop.  Only an arc that leaves a seed can carry anything in one hop, so the
    restatement of a set gets those arcs alone."""
    s = lc.FWD_PUSH
    n, pairs, sets, prob = forward_push()
    rows = []
    for seeds in sets:
        keep = np.isin(pairs[:, 0], seeds)
        if arcs:
            rows.append(arc.spread_trials_arcs(n, pairs[keep], True, prob[keep], seeds, s["T"], IC_SEED, 1))
        else:
            rows.append(ic.spread_trials(n, pairs[keep], True, seeds, s["p"], s["T"], IC_SEED, 1))
    return np.array(rows)


# ---- C: reverse sampling, pull at W > 16 ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reverse_pull():
    s = lc.REV_PULL
    return s["n"], ic.canonical_arcs(s["n"], gr.random_regular_edges(s["n"] - 3, s["degree"], seed=2), False)


@functools.lru_cache(maxsize=None)
def reverse_pull_expected():
    """((indptr, members, roots), Frontiers by chunk of the words gh_ic_rr_sample takes at a time)."""
    s = lc.REV_PULL
    n, pairs = reverse_pull()
    f = ic.Frontiers(lc.rr_words_per_chunk(lc.defines(), n, s["samples"]))
    return ris.rr_sets(n, pairs, False, s["p"], s["samples"], IC_SEED, s["hops"], frontiers=f), f


# ---- D: reverse push at W = 128 ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reverse_push():
    """(n, canonical pairs, trials, roots, (A,) probabilities): in-degree 3 on all but the three isolated vertices;
    `distinct_roots` roots, one of them isolated, and the other samples on roots that are taken already; repeated trials."""
    s = lc.REV_PUSH
    n = s["n"]
    rng = np.random.default_rng(29)
    pairs = ic.canonical_arcs(n, _out_regular(n - 3, s["in_degree"], rng)[:, ::-1], True)
    distinct = rng.choice(n - 3, s["distinct_roots"], replace=False)
    distinct[0] = n - 2
    roots = rng.permutation(np.concatenate([distinct, rng.choice(distinct, s["samples"] - s["distinct_roots"])]))
    trials = rng.integers(0, 2 ** 40, s["samples"]).astype(np.uint64)
    trials[100:140] = trials[99]
    prob = arc.mixed_probabilities(rng, len(pairs), s["arc_scale"])
    return n, pairs, trials, roots, prob


@functools.lru_cache(maxsize=None)
def reverse_push_expected(arcs):
    """(indptr, members, roots) after one hop, from the arcs whose head is a root: no other arc is walked."""
    s = lc.REV_PUSH
    n, pairs, trials, roots, prob = reverse_push()
    keep = np.isin(pairs[:, 1], roots)
    if arcs:
        return arc.rr_sets_arcs(n, pairs[keep], True, prob[keep], seed=IC_SEED, max_hops=1, trials=trials, roots=roots)
    return ris.rr_sets(n, pairs[keep], True, s["p"], seed=IC_SEED, max_hops=1, trials=trials, roots=roots)


# ---- E: the coverage kernels on an uploaded system -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cover_system():
    """(n, indptr, members): set sizes from COVER['sizes']; the heavy vertex, above the first trip of rr_argmax_kernel, in
    every third set and in no other; and two vertices, one on each side of that trip, each in `tie_sets` sets of its own
    that the heavy vertex is not in -- once it is taken the two lead with equal counts."""
    s = lc.COVER
    n, S = s["n"], s["sets"]
    rng = np.random.default_rng(31)
    sizes = rng.choice(s["sizes"], size=S)
    special = (s["heavy"], s["tie_low"], s["tie_high"])
    sets = []
    for j in range(S):
        m = rng.choice(n, int(sizes[j]), replace=False)
        m = m[~np.isin(m, special)]
        if j % 3 == 0:
            m = np.append(m, s["heavy"])
        elif j < 3 * s["tie_sets"]:
            m = np.append(m, s["tie_low"] if j % 3 == 1 else s["tie_high"])
        sets.append(np.sort(m))
    indptr = np.zeros(S + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(m) for m in sets])
    return n, indptr, np.concatenate(sets).astype(np.int32)


@functools.lru_cache(maxsize=None)
def cover_expected(k):
    n, indptr, members = cover_system()
    return ris.max_coverage(indptr, members, n, k)
