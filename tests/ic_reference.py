"""numpy restatement of the Independent Cascade coin rule of include/graphem_hip.h (the checker of gh_ic_spread).

In trial t the pair (a, b) is live iff coin(seed, t, a, b) < thr; the reached set of trial t is the breadth-first search
over the live arcs from the seeds, cut at max_hops.  Trials are evaluated 64 at a time as bit masks, like the kernel.
"""
import numpy as np

G = np.uint64(0x9E3779B97F4A7C15)
M1, M2 = np.uint64(0xbf58476d1ce4e5b9), np.uint64(0x94d049bb133111eb)


def mix(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * M1
        z = (z ^ (z >> np.uint64(27))) * M2
    return z ^ (z >> np.uint64(31))


def threshold(p):
    return min(1 << 24, int(np.floor(p * 16777216.0 + 0.5)))


def canonical_arcs(n, arcs, directed):
    """(A, 2) int64 unique arcs without self-loops; an undirected edge as (min, max)."""
    arcs = np.asarray(arcs, dtype=np.int64).reshape(-1, 2)
    arcs = arcs[arcs[:, 0] != arcs[:, 1]]
    if not directed:
        arcs = np.sort(arcs, axis=1)
    return np.unique(arcs, axis=0) if len(arcs) else arcs


class Frontiers:
    """What the restatements see of the level machinery's work lists, for tests/launch_caps.py: per chunk of
    `words_per_chunk` words (None: one chunk) and level r, the vertices whose frontier word of round r + 1 is non-zero in
    any word, and the vertices that are visited in any word at the end (the touched list)."""

    def __init__(self, words_per_chunk=None):
        self.words_per_chunk = words_per_chunk
        self.levels, self.touched = {}, {}

    def _chunk(self, w):
        return 0 if self.words_per_chunk is None else w // self.words_per_chunk

    def level(self, w, r, front):
        rows = self.levels.setdefault(self._chunk(w), [])
        if r == len(rows):
            rows.append(np.zeros(len(front), dtype=bool))
        rows[r] |= front != 0

    def done(self, w, vis):
        c = self._chunk(w)
        self.touched[c] = (vis != 0) | self.touched.get(c, False)

    def entries(self, chunk=0):
        """Frontier entries of every level that had any: what *cur_cnt holds in round 1, 2, ..."""
        return [int(x.sum()) for x in self.levels.get(chunk, [])]

    def touched_entries(self, chunk=0):
        return int(np.sum(self.touched.get(chunk, 0)))


def spread_trials(n, arcs, directed, seeds, p, n_trials, seed=0, max_hops=None, frontiers=None):
    """(n_trials,) int64: the spread of every trial.  frontiers: a Frontiers that records the levels on the way."""
    pairs = canonical_arcs(n, arcs, directed)
    src, dst = pairs[:, 0], pairs[:, 1]
    if not directed:   # both directions share the pair's coin
        src, dst, pairs = np.concatenate([src, dst]), np.concatenate([dst, src]), np.concatenate([pairs, pairs])
    key = (pairs[:, 0].astype(np.uint64) << np.uint64(32)) | pairs[:, 1].astype(np.uint64)
    order = np.argsort(dst, kind="stable")
    src, dst, key = src[order], dst[order], key[order]
    starts = np.flatnonzero(np.r_[True, dst[1:] != dst[:-1]]) if len(dst) else np.zeros(0, dtype=np.int64)
    thr = np.uint64(threshold(p))
    seeds = np.unique(np.asarray(seeds, dtype=np.int64))
    hops = n if max_hops is None else max_hops
    out = np.zeros(n_trials, dtype=np.int64)
    bits = np.uint64(1) << np.arange(64, dtype=np.uint64)
    for w in range((n_trials + 63) // 64):
        t = np.arange(64 * w, min(64 * w + 64, n_trials), dtype=np.uint64)
        valid = np.uint64((1 << len(t)) - 1) if len(t) < 64 else np.uint64(0xFFFFFFFFFFFFFFFF)
        with np.errstate(over="ignore"):
            h = mix(np.uint64(seed) + t * G)
        live_bits = (mix(h[None, :] ^ key[:, None]) >> np.uint64(40)) < thr          # (arcs, trials)
        live = np.bitwise_or.reduce(np.where(live_bits, bits[:len(t)], np.uint64(0)), axis=1) if len(key) else key
        vis = np.zeros(n, dtype=np.uint64)
        vis[seeds] = valid
        front = vis.copy()
        for r in range(hops):
            if not front.any() or len(key) == 0:
                break
            if frontiers is not None:
                frontiers.level(w, r, front)
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
