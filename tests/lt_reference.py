"""numpy restatement of the Linear Threshold rule of include/graphem_hip.h (the checker of gh_ic_set_lt_weights,
gh_ic_spread_lt and gh_ic_rr_sample_lt), and two independent checkers of the rule itself.

In trial t vertex v selects the in-arc whose interval [lo, hi) of v's row holds pick(seed, t, v) -- at most one; the
selected arcs are the live digraph of the trial, a cascade is the breadth-first search over it from the seeds, cut at
max_hops, and an RR set the search backwards from the root.  Trials are evaluated 64 at a time as bit masks, like the
kernels.  weight has the shape influence.lt_weights returns for the canonical pairs: (A,) for a directed graph, (A, 2) --
a -> b, b -> a -- for an undirected one.

exact_moments enumerates every selection of a tiny graph; threshold_process simulates the threshold model itself (theta_v
uniform, synchronous rounds), which the live-edge form is claimed to equal round for round (Kempe et al. 2003, Claim 2.6).
"""
import itertools

import numpy as np

from arc_ic_reference import as_directed
from ic_reference import G, canonical_arcs, mix
from ris_reference import default_roots

TWO32 = 4294967296.0
ROW_MARGIN = 1.0 + 2.0 ** -20


def lt_intervals(n, src, dst, w):
    """(src, dst, lo, hi), by (target, source) ascending, of the DIRECTED arcs src -> dst with weights w, given in any
    order: S_k the sequential double sum of the first k weights of a row, c_k = min(2^32 - 1, floor(S_k 2^32 + 0.5)), and
    the k-th in-arc has [c_{k-1}, c_k).  lo and hi are uint64 holding 32-bit values.  ValueError for a weight that is NaN
    or outside [0, 1], a repeated pair, a loop, and a row whose sum is above 1 + 2^-20."""
    src, dst = np.asarray(src, dtype=np.int64).ravel(), np.asarray(dst, dtype=np.int64).ravel()
    w = np.asarray(w, dtype=np.float64).ravel()
    assert len(src) == len(dst) == len(w)
    if len(w) and not (np.all(w >= 0.0) and np.all(w <= 1.0)):
        raise ValueError("weights must lie in [0, 1] and must not be NaN")
    if (src == dst).any():
        raise ValueError("a self-loop has no weight")
    order = np.lexsort((src, dst))
    src, dst, w = src[order], dst[order], w[order]
    if len(src) > 1 and ((src[1:] == src[:-1]) & (dst[1:] == dst[:-1])).any():
        raise ValueError("a pair is listed twice")
    first = np.r_[True, dst[1:] != dst[:-1]] if len(dst) else np.zeros(0, dtype=bool)
    start = np.flatnonzero(first)
    pos = np.arange(len(dst)) - np.repeat(start, np.diff(np.r_[start, len(dst)]))
    S = np.zeros(len(w))
    run = np.zeros(n)
    by_pos = np.argsort(pos, kind="stable")
    cuts = np.searchsorted(pos[by_pos], np.arange(int(pos.max()) + 2)) if len(pos) else [0]
    for k in range(len(cuts) - 1):          # the k-th arc of every row that has one: sequential within a row
        idx = by_pos[cuts[k]:cuts[k + 1]]
        run[dst[idx]] += w[idx]
        S[idx] = run[dst[idx]]
    if len(run) and run.max() > ROW_MARGIN:
        v = int(np.argmax(run > ROW_MARGIN))
        raise ValueError(f"the weights into vertex {v} sum to {run[v]!r}, above 1 + 2^-20")
    hi = np.minimum(TWO32 - 1.0, np.floor(S * TWO32 + 0.5)).astype(np.uint64)
    lo = np.r_[np.uint64(0), hi[:-1]].astype(np.uint64) if len(hi) else hi
    lo[first] = 0
    return src, dst, lo, hi


def rows_of(n, pairs, directed, weight):
    """lt_intervals of canonical pairs and lt_weights' array."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    assert np.array_equal(pairs, canonical_arcs(n, pairs, directed)), "pairs must be the canonical arc array"
    weight = np.asarray(weight, dtype=np.float64)
    assert weight.shape == ((len(pairs),) if directed else (len(pairs), 2))
    arcs, w = as_directed(pairs, directed, weight)
    return lt_intervals(n, arcs[:, 0], arcs[:, 1], w)


def _live(h, dst, lo, hi, bits):
    """The live mask of every arc over the trials of h: the pick of the arc's target against the arc's interval."""
    if len(dst) == 0:
        return np.zeros(0, dtype=np.uint64)
    key = (dst.astype(np.uint64) << np.uint64(32)) | dst.astype(np.uint64)
    pick = mix(h[None, :] ^ key[:, None]) >> np.uint64(32)                            # (arcs, trials)
    live_bits = (pick >= lo[:, None]) & (pick < hi[:, None])
    return np.bitwise_or.reduce(np.where(live_bits, bits[:len(h)], np.uint64(0)), axis=1)


def spread_trials_lt(n, pairs, directed, weight, seeds, n_trials, seed=0, max_hops=None, frontiers=None, rows=None):
    """(n_trials,) int64: the spread of every trial.  frontiers: an ic_reference.Frontiers that records the levels.
    rows: arcs with their intervals, by target, in place of pairs and weight -- a subset of rows_of of the whole graph,
    where the other arcs are known to carry nothing."""
    src, dst, lo, hi = rows_of(n, pairs, directed, weight) if rows is None else rows   # by target: reduceat over a row
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
        live = _live(h, dst, lo, hi, bits)
        vis = np.zeros(n, dtype=np.uint64)
        vis[seeds] = valid
        front = vis.copy()
        for level in range(hops):
            if not front.any() or len(dst) == 0:
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


def rr_sets_lt(n, pairs, directed, weight, n_samples=None, seed=0, max_hops=None, trials=None, roots=None, frontiers=None,
               rows=None):
    """(indptr int64, members int32, roots int32): the RR sets of the samples, members ascending within a set.  rows: as
    for spread_trials_lt."""
    if trials is None:
        trials = np.arange(n_samples, dtype=np.uint64)
    trials = np.asarray(trials, dtype=np.uint64)
    roots = default_roots(n, seed, trials) if roots is None else np.asarray(roots, dtype=np.int64)
    S = len(trials)
    src, dst, lo, hi = rows_of(n, pairs, directed, weight) if rows is None else rows
    order = np.argsort(src, kind="stable")   # backwards: an arc src -> dst carries dst's bits to src
    src, dst, lo, hi = src[order], dst[order], lo[order], hi[order]
    starts = np.flatnonzero(np.r_[True, src[1:] != src[:-1]]) if len(src) else np.zeros(0, dtype=np.int64)
    hops = n if max_hops is None else max_hops
    bits = np.uint64(1) << np.arange(64, dtype=np.uint64)
    sets = []
    for w in range((S + 63) // 64):
        t = trials[64 * w:64 * w + 64]
        r = roots[64 * w:64 * w + 64]
        with np.errstate(over="ignore"):
            h = mix(np.uint64(seed) + t * G)
        live = _live(h, dst, lo, hi, bits)
        vis = np.zeros(n, dtype=np.uint64)
        np.bitwise_or.at(vis, r, bits[:len(t)])
        front = vis.copy()
        for level in range(hops):
            if not front.any() or len(src) == 0:
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


def _widths(rows):
    src, dst, lo, hi = rows
    return src, dst, (hi.astype(np.float64) - lo.astype(np.float64)) / TWO32


def exact_moments(n, rows, seeds, hops=None):
    """(mean, standard deviation) of the spread over ALL selections of a tiny graph: every vertex takes one of its in-arcs
    with probability (c_k - c_{k-1}) / 2^32 or none with the rest, independently.  rows: what lt_intervals returns."""
    src, dst, q = _widths(rows)
    targets = np.unique(dst)
    options = []                             # per target: [(source or -1, probability), ...]
    for v in targets:
        k = np.flatnonzero(dst == v)
        options.append([(int(src[i]), float(q[i])) for i in k] + [(-1, 1.0 - float(q[k].sum()))])
    assert np.prod([len(o) for o in options], dtype=np.float64) <= 1 << 20
    seeds = sorted({int(s) for s in seeds})
    mean = second = total = 0.0
    for choice in itertools.product(*options):
        prob = float(np.prod([c[1] for c in choice]))
        if prob == 0.0:
            continue
        chosen = {int(v): c[0] for v, c in zip(targets, choice) if c[0] >= 0}      # target -> its one live source
        reached, front = set(seeds), set(seeds)
        for _ in range(n if hops is None else hops):
            front = {v for v, u in chosen.items() if u in front and v not in reached}
            if not front:
                break
            reached |= front
        total += prob
        mean += prob * len(reached)
        second += prob * len(reached) ** 2
    assert abs(total - 1.0) < 1e-12
    return mean, float(np.sqrt(max(0.0, second - mean * mean)))


def threshold_process(n, rows, seeds, hops, n_trials, rng):
    """(n_trials,) int64: active vertices after `hops` synchronous rounds (None: until nothing changes) of the threshold
    model itself -- theta_v uniform on (0, 1] from rng, the seeds active at round 0, and v active from the round on in
    which the weights of its active in-neighbours reach theta_v.  The weights are the interval widths of rows."""
    src, dst, q = _widths(rows)
    W = np.zeros((n, n))
    W[src, dst] = q
    theta = 1.0 - rng.random((n_trials, n))   # (0, 1]: a vertex nobody influences never reaches its threshold
    active = np.zeros((n_trials, n), dtype=bool)
    active[:, np.unique(np.asarray(list(seeds), dtype=np.int64))] = True
    for _ in range(n if hops is None else hops):
        grown = active | (active.astype(np.float64) @ W >= theta)
        if np.array_equal(grown, active):
            break
        active = grown
    return active.sum(axis=1).astype(np.int64)


def mixed_weights(seed, n, pairs, directed):
    """A weight table in lt_weights' shape whose rows, by target id modulo 5, (0) sum exactly to 1 (equal dyadic weights),
    (1) stay well below 1, (2) have exact zeros among random weights, (3) put weight 1 on a single arc, and (4) start
    with 2^-33 twice: the first gets the one-value interval [0, 1), the second -- S = 2^-32 rounds to the same bound --
    an empty one, a positive weight nobody can select."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    rng = np.random.default_rng(seed)
    arcs = pairs if directed else np.concatenate([pairs, pairs[:, ::-1]])
    order = np.lexsort((arcs[:, 0], arcs[:, 1]))
    w = np.zeros(len(arcs))
    dst = arcs[order, 1]
    start = np.flatnonzero(np.r_[True, dst[1:] != dst[:-1]]) if len(dst) else np.zeros(0, dtype=np.int64)
    for b, e in zip(start, np.r_[start[1:], len(dst)]):
        d, kind = int(e - b), int(dst[b]) % 5
        if kind == 0:
            p2 = 1 << (d.bit_length() - 1)            # 1 / p2 on p2 of the arcs: every partial sum is exact
            row = rng.permutation(np.r_[np.full(p2, 1.0 / p2), np.zeros(d - p2)])
        elif kind == 1:
            row = rng.random(d) * 0.5 / d
        elif kind == 2:
            row = rng.random(d) / d
            row[rng.random(d) < 0.5] = 0.0
        elif kind == 3:
            row = np.zeros(d)
            row[rng.integers(d)] = 1.0
        else:
            row = rng.random(d) * 0.9 / d
            row[:2] = 2.0 ** -33
        w[order[b:e]] = row
    return w if directed else np.column_stack([w[:len(pairs)], w[len(pairs):]])
