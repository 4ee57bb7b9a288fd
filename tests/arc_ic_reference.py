"""numpy restatement of the per-arc Independent Cascade rule of include/graphem_hip.h (the checker of gh_ic_spread_arcs and
gh_ic_rr_sample_arcs), and the exact moments of the spread under independent coins per directed arc.

Arc u -> v is live in trial t iff coin(seed, t, a, b) < thr_uv: the coin and its key (a, b) are those of ic_reference --
(u, v) for a directed graph, (min, max) for an undirected one, whose two directions share the coin -- and only the
threshold is the arc's own.  prob has the shape influence.arc_probabilities returns for the canonical pairs: (A,) for a
directed graph, (A, 2) -- a -> b, b -> a -- for an undirected one.
"""
import numpy as np

from ic_reference import G, canonical_arcs, mix, threshold
from ris_reference import default_roots


def mixed_probabilities(rng, shape, scale=1.0):
    """Random probabilities with exact 0, exact 1, 1e-9 (threshold 0) and 1 - 1e-9 (threshold 2^24) mixed in."""
    prob = rng.random(shape) * scale
    kind = rng.integers(0, 20, shape)
    for k, value in enumerate((0.0, 1.0, 1e-9, 1.0 - 1e-9)):
        prob[kind == k] = value
    assert all((prob == v).any() for v in (0.0, 1.0, 1e-9, 1.0 - 1e-9))
    return prob


def _live_arcs(n, pairs, directed, prob):
    """(src, dst, key, thr) of every directed arc, for canonical `pairs`."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    assert np.array_equal(pairs, canonical_arcs(n, pairs, directed)), "pairs must be the canonical arc array"
    prob = np.asarray(prob, dtype=np.float64)
    assert prob.shape == ((len(pairs),) if directed else (len(pairs), 2))
    src, dst = pairs[:, 0], pairs[:, 1]
    if not directed:   # both directions share the pair's coin; each has its own threshold
        src, dst, pairs = np.concatenate([src, dst]), np.concatenate([dst, src]), np.concatenate([pairs, pairs])
        prob = np.concatenate([prob[:, 0], prob[:, 1]])
    key = (pairs[:, 0].astype(np.uint64) << np.uint64(32)) | pairs[:, 1].astype(np.uint64)
    thr = np.array([threshold(x) for x in prob], dtype=np.uint64)
    return src, dst, key, thr


def spread_trials_arcs(n, pairs, directed, prob, seeds, n_trials, seed=0, max_hops=None, frontiers=None):
    """(n_trials,) int64: the spread of every trial (ic_reference.spread_trials with a threshold per arc)."""
    src, dst, key, thr = _live_arcs(n, pairs, directed, prob)
    order = np.argsort(dst, kind="stable")
    src, dst, key, thr = src[order], dst[order], key[order], thr[order]
    starts = np.flatnonzero(np.r_[True, dst[1:] != dst[:-1]]) if len(dst) else np.zeros(0, dtype=np.int64)
    seeds = np.unique(np.asarray(seeds, dtype=np.int64))
    hops = n if max_hops is None else max_hops
    out = np.zeros(n_trials, dtype=np.int64)
    bits = np.uint64(1) << np.arange(64, dtype=np.uint64)
    for w in range((n_trials + 63) // 64):
        t = np.arange(64 * w, min(64 * w + 64, n_trials), dtype=np.uint64)
        valid = np.uint64((1 << len(t)) - 1) if len(t) < 64 else np.uint64(0xFFFFFFFFFFFFFFFF)
        with np.errstate(over="ignore"):
            h = mix(np.uint64(seed) + t * G)
        live_bits = (mix(h[None, :] ^ key[:, None]) >> np.uint64(40)) < thr[:, None]          # (arcs, trials)
        live = np.bitwise_or.reduce(np.where(live_bits, bits[:len(t)], np.uint64(0)), axis=1) if len(key) else key
        vis = np.zeros(n, dtype=np.uint64)
        vis[seeds] = valid
        front = vis.copy()
        for level in range(hops):
            if not front.any() or len(key) == 0:
                break
            if frontiers is not None:
                frontiers.level(w, level, front)
            contrib = front[src] & live
            nxt = np.zeros(n, dtype=np.uint64)
            nxt[dst[starts]] = np.bitwise_or.reduceat(contrib, starts)
            nxt &= ~vis
            vis |= nxt
            front = nxt
        if frontiers is not None:
            frontiers.done(w, vis)
        for j in range(len(t)):
            out[64 * w + j] = int(np.count_nonzero(vis & bits[j]))
    return out


def rr_sets_arcs(n, pairs, directed, prob, n_samples=None, seed=0, max_hops=None, trials=None, roots=None, frontiers=None):
    """(indptr int64, members int32, roots int32): ris_reference.rr_sets with a threshold per arc."""
    if trials is None:
        trials = np.arange(n_samples, dtype=np.uint64)
    trials = np.asarray(trials, dtype=np.uint64)
    roots = default_roots(n, seed, trials) if roots is None else np.asarray(roots, dtype=np.int64)
    S = len(trials)
    src, dst, key, thr = _live_arcs(n, pairs, directed, prob)
    order = np.argsort(src, kind="stable")   # backwards: an arc src -> dst carries dst's bits to src
    src, dst, key, thr = src[order], dst[order], key[order], thr[order]
    starts = np.flatnonzero(np.r_[True, src[1:] != src[:-1]]) if len(src) else np.zeros(0, dtype=np.int64)
    hops = n if max_hops is None else max_hops
    bits = np.uint64(1) << np.arange(64, dtype=np.uint64)
    sets = []
    for w in range((S + 63) // 64):
        t = trials[64 * w:64 * w + 64]
        r = roots[64 * w:64 * w + 64]
        with np.errstate(over="ignore"):
            h = mix(np.uint64(seed) + t * G)
        live_bits = (mix(h[None, :] ^ key[:, None]) >> np.uint64(40)) < thr[:, None]          # (arcs, samples)
        live = np.bitwise_or.reduce(np.where(live_bits, bits[:len(t)], np.uint64(0)), axis=1) if len(key) else key
        vis = np.zeros(n, dtype=np.uint64)
        np.bitwise_or.at(vis, r, bits[:len(t)])
        front = vis.copy()
        for level in range(hops):
            if not front.any() or len(key) == 0:
                break
            if frontiers is not None:
                frontiers.level(w, level, front)
            contrib = front[dst] & live
            nxt = np.zeros(n, dtype=np.uint64)
            nxt[src[starts]] = np.bitwise_or.reduceat(contrib, starts)
            nxt &= ~vis
            vis |= nxt
            front = nxt
        if frontiers is not None:
            frontiers.done(w, vis)
        reached = np.flatnonzero(vis)   # ascending, so every set's members are
        words = vis[reached]
        for j in range(len(t)):
            sets.append(reached[(words & bits[j]) != 0].astype(np.int32))
    indptr = np.zeros(S + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(s) for s in sets])
    members = np.concatenate(sets) if sets else np.zeros(0, dtype=np.int32)
    return indptr, members.astype(np.int32), roots.astype(np.int32)


def as_directed(pairs, directed, prob):
    """((D, 2) directed arcs, (D,) probabilities) of canonical pairs and arc_probabilities' array: what exact_moments takes."""
    pairs, prob = np.asarray(pairs, dtype=np.int64).reshape(-1, 2), np.asarray(prob, dtype=np.float64)
    if directed:
        return pairs, prob
    return np.concatenate([pairs, pairs[:, ::-1]]), np.concatenate([prob[:, 0], prob[:, 1]])


def exact_moments(n, directed_arcs, probs, seeds, max_hops=None):
    """(mean, variance) of the spread when every DIRECTED arc has an independent coin of probability thr / 2^24: the sum
    over all 2^D live-arc subsets (D up to about 14) of the subset's probability times the breadth-first count."""
    arcs = np.asarray(directed_arcs, dtype=np.int64).reshape(-1, 2)
    q = np.array([threshold(x) for x in probs], dtype=np.float64) / 16777216.0
    D = len(arcs)
    assert D <= 16
    subsets = np.arange(1 << D, dtype=np.int64)
    live = ((subsets[:, None] >> np.arange(D)) & 1).astype(bool)                   # (2^D, D)
    weight = np.prod(np.where(live, q, 1.0 - q), axis=1)
    vis = np.zeros((1 << D, n), dtype=bool)
    vis[:, np.unique(np.asarray(seeds, dtype=np.int64))] = True
    front = vis.copy()
    for _ in range(n if max_hops is None else max_hops):
        nxt = np.zeros_like(vis)
        for j, (u, v) in enumerate(arcs):
            nxt[:, v] |= front[:, u] & live[:, j]
        nxt &= ~vis
        if not nxt.any():
            break
        vis |= nxt
        front = nxt
    count = vis.sum(axis=1).astype(np.float64)
    mean = float(np.dot(weight, count))
    return mean, float(np.dot(weight, (count - mean) ** 2))
