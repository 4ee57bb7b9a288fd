"""The hop-profile rule of include/graphem_hip.h ("distance preservation") restated in numpy, for the tests: the simple
graph of tests/neighbors_reference.py, a plain breadth-first search per source, the float32 distance chain of
neighbors_reference.dist2_from, every term (sqrt, the quotients by hop and hop^2) formed in np.longdouble and rounded to
double once, and the terms summed with math.fsum, which is exact on the doubles it is given.  A sum here is therefore
within one rounding per term of the true sum.  Nothing of the package is imported."""
import math

import numpy as np

import neighbors_reference as nref


def hop_distances(n, indptr, indices, s):
    """int64 hop(s, v) for every v; -1 where v is not reached."""
    dist = np.full(n, -1, dtype=np.int64)
    dist[s] = 0
    frontier, level = [int(s)], 0
    while frontier:
        level += 1
        nxt = []
        for u in frontier:
            for v in indices[indptr[u]:indptr[u + 1]].tolist():
                if dist[v] < 0:
                    dist[v] = level
                    nxt.append(v)
        frontier = nxt
    return dist


def all_hops(n, edges):
    """(n, n) int64: row s = hop_distances from s.  The searches do not depend on the positions, so tests share them."""
    gp, gi = nref.simple_graph(n, edges)
    return np.array([hop_distances(n, gp, gi, s) for s in range(n)], dtype=np.int64).reshape(n, n)


def _fsum(terms):
    return math.fsum(np.asarray(terms, dtype=np.float64).tolist())


def hop_profile(pos, edges, sources=None, hops=None):
    """dict of sources (int64), the per-hop arrays (entry h - 1 for hop h: pairs int64, sum_d, sum_d2 float64, min_d2, max_d2
    float32) and the per-source arrays (reach int64, eccentricity int32, sum_d_over_h, sum_d2_over_h2 float64).  hops: the
    matrix of all_hops, when the caller has it."""
    pos = np.asarray(pos, dtype=np.float32)
    n = len(pos)
    gp, gi = nref.simple_graph(n, edges)
    sources = np.arange(n, dtype=np.int64) if sources is None else np.asarray(sources, dtype=np.int64).ravel()
    S = len(sources)
    reach, ecc = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int32)
    over_h, over_h2 = np.zeros(S), np.zeros(S)
    level, dist2 = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.float32)]
    for j, s in enumerate(sources.tolist()):
        hop = hop_distances(n, gp, gi, s) if hops is None else hops[s]
        at = hop > 0
        reach[j] = int(at.sum())
        if reach[j] == 0:
            continue
        ecc[j] = hop.max()
        d2 = nref.dist2_from(pos, s)[at]
        with np.errstate(all="ignore"):
            q, h = d2.astype(np.longdouble), hop[at].astype(np.longdouble)
            over_h[j] = _fsum(np.sqrt(q) / h)
            over_h2[j] = _fsum(q / (h * h))
        level.append(hop[at])
        dist2.append(d2)
    level, dist2 = np.concatenate(level), np.concatenate(dist2)
    H = int(level.max()) if len(level) else 0
    out = {"sources": sources.copy(), "pairs": np.zeros(H, dtype=np.int64), "sum_d": np.zeros(H), "sum_d2": np.zeros(H),
           "min_d2": np.zeros(H, dtype=np.float32), "max_d2": np.zeros(H, dtype=np.float32),
           "reach": reach, "eccentricity": ecc, "sum_d_over_h": over_h, "sum_d2_over_h2": over_h2}
    for l in range(1, H + 1):
        d2 = dist2[level == l]
        out["pairs"][l - 1] = len(d2)
        with np.errstate(all="ignore"):
            out["sum_d"][l - 1] = _fsum(np.sqrt(d2.astype(np.longdouble)))
            out["sum_d2"][l - 1] = _fsum(d2)
            out["min_d2"][l - 1], out["max_d2"][l - 1] = d2.min(), d2.max()
    return out


def close(got, want, terms):
    """The comparison rule for a double sum of `terms` non-negative terms: relative (terms + 8) 2^-52 against the reference,
    and exactly 0 without terms."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False
    terms = np.broadcast_to(np.asarray(terms, dtype=np.float64), want.shape)
    return bool(np.all(np.where(terms == 0, got == 0, np.abs(got - want) <= (terms + 8) * 2.0 ** -52 * np.abs(want))))
