"""numpy restatement of the reverse-influence-sampling rule of include/graphem_hip.h (the checker of gh_ic_rr_sample,
gh_rr_cover and gh_rr_count_hit).

Sample j is (trial t_j, root r_j); RR(t, r) is the breadth-first search from r that walks every arc backwards over the
live arcs of trial t, cut at max_hops.  Samples are evaluated 64 at a time as bit masks, like the kernel: bit b of a word
is sample 64w + b, and every bit has its own trial.
"""
import numpy as np

from ic_reference import G, canonical_arcs, mix, threshold

ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def default_roots(n, seed, trials):
    """r = ((mix(mix(seed + t * G) ^ ones) >> 32) * n) >> 32 for every trial."""
    t = np.asarray(trials, dtype=np.uint64)
    with np.errstate(over="ignore"):
        w = mix(mix(np.uint64(seed) + t * G) ^ ONES)
    return (((w >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def rr_sets(n, arcs, directed, p, n_samples=None, seed=0, max_hops=None, trials=None, roots=None, frontiers=None):
    """(indptr int64, members int32, roots int32): the RR sets of the samples, members ascending within a set."""
    if trials is None:
        trials = np.arange(n_samples, dtype=np.uint64)
    trials = np.asarray(trials, dtype=np.uint64)
    roots = default_roots(n, seed, trials) if roots is None else np.asarray(roots, dtype=np.int64)
    S = len(trials)
    pairs = canonical_arcs(n, arcs, directed)
    src, dst = pairs[:, 0], pairs[:, 1]
    if not directed:   # both directions share the pair's coin
        src, dst, pairs = np.concatenate([src, dst]), np.concatenate([dst, src]), np.concatenate([pairs, pairs])
    key = (pairs[:, 0].astype(np.uint64) << np.uint64(32)) | pairs[:, 1].astype(np.uint64)
    order = np.argsort(src, kind="stable")   # backwards: an arc src -> dst carries dst's bits to src
    src, dst, key = src[order], dst[order], key[order]
    starts = np.flatnonzero(np.r_[True, src[1:] != src[:-1]]) if len(src) else np.zeros(0, dtype=np.int64)
    thr = np.uint64(threshold(p))
    hops = n if max_hops is None else max_hops
    bits = np.uint64(1) << np.arange(64, dtype=np.uint64)
    sets = []
    for w in range((S + 63) // 64):
        t = trials[64 * w:64 * w + 64]
        r = roots[64 * w:64 * w + 64]
        with np.errstate(over="ignore"):
            h = mix(np.uint64(seed) + t * G)
        live_bits = (mix(h[None, :] ^ key[:, None]) >> np.uint64(40)) < thr          # (arcs, samples)
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


def max_coverage(indptr, members, n, k):
    """(seeds, gains): min(k, n) rounds; each takes the unchosen vertex in the most uncovered sets, ties to the smallest id."""
    indptr, members = np.asarray(indptr, dtype=np.int64), np.asarray(members, dtype=np.int64)
    set_of = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    covered = np.zeros(len(indptr) - 1, dtype=bool)
    chosen = np.zeros(n, dtype=bool)
    seeds, gains = [], []
    for _ in range(min(int(k), n)):
        live = ~covered[set_of]
        count = np.bincount(members[live], minlength=n)
        count[chosen] = -1
        v = int(np.argmax(count))          # first maximum = smallest id
        seeds.append(v)
        gains.append(int(count[v]))
        chosen[v] = True
        covered[set_of[members == v]] = True
    return seeds, np.array(gains, dtype=np.int64)


def count_hit(indptr, members, vertices):
    indptr, members = np.asarray(indptr, dtype=np.int64), np.asarray(members, dtype=np.int64)
    set_of = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    return int(len(np.unique(set_of[np.isin(members, np.asarray(list(vertices), dtype=np.int64))])))


class Collections:
    """The three callables of influence.opim_c over this restatement (R1 on the even trials, R2 on the odd ones)."""

    def __init__(self, n, arcs, directed, p, seed, max_hops=None):
        self.args = (n, arcs, directed, p)
        self.n, self.seed, self.hops = n, seed, max_hops
        self.r1 = self.r2 = None
        self.thetas = []

    def sample(self, theta):
        self.thetas.append(theta)
        ev = 2 * np.arange(theta, dtype=np.uint64)
        self.r1 = rr_sets(*self.args, seed=self.seed, max_hops=self.hops, trials=ev)
        self.r2 = rr_sets(*self.args, seed=self.seed, max_hops=self.hops, trials=ev + np.uint64(1))

    def cover(self, k):
        return max_coverage(self.r1[0], self.r1[1], self.n, k)

    def count(self, seeds):
        return count_hit(self.r2[0], self.r2[1], seeds)
