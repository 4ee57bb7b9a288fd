"""The neighbour-rank rule of include/graphem_hip.h ("embedding quality") restated in numpy, for the tests.  The float32
chain is written as separate numpy float32 operations in coordinate order (numpy rounds every operation to the array's
type and contracts nothing); the counts are direct comparisons over all w; the simple graph is rebuilt here; the metrics
are written with Python integers and one division each.  Nothing of the package is imported."""
import math

import numpy as np


def simple_graph(n, edges):
    """(indptr int64, indices int32) of the simple undirected graph: self-loops dropped, repeats and both directions merged,
    each row's ids ascending."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    e = e[e[:, 0] != e[:, 1]]
    both = np.unique(np.concatenate([e, e[:, ::-1]]), axis=0) if len(e) else np.zeros((0, 2), dtype=np.int64)   # sorted by (u, v)
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(both[:, 0], minlength=n), out=indptr[1:])
    return indptr, both[:, 1].astype(np.int32)


def dist2_from(pos, u):
    """float32 d2(u, w) for every w: (((0 + t_0 t_0) + t_1 t_1) + ...), t_d = x[u][d] - x[w][d]."""
    pos = np.asarray(pos, dtype=np.float32)
    s = np.zeros(len(pos), dtype=np.float32)
    with np.errstate(all="ignore"):
        for d in range(pos.shape[1]):
            t = pos[u, d] - pos[:, d]
            s = s + t * t
    assert s.dtype == np.float32
    s[np.isnan(s)] = np.float32(np.nan)   # the rule returns every NaN as 0x7FC00000: sign and payload are no part of it
    return s


def neighbor_ranks(pos, edges, rows=None):
    """dict(sources, indptr, neighbors, dist2, below, equal) over `rows` (None: every vertex in order); counts int64."""
    pos = np.asarray(pos, dtype=np.float32)
    n = len(pos)
    gp, gi = simple_graph(n, edges)
    rows = np.arange(n, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64).ravel()
    indptr = np.zeros(len(rows) + 1, dtype=np.int64)
    nbrs, d2s, below, equal = [], [], [], []
    for r, u in enumerate(rows):
        nb = gi[gp[u]:gp[u + 1]]
        indptr[r + 1] = indptr[r] + len(nb)
        if len(nb) == 0:
            continue
        d = dist2_from(pos, u)
        others = np.ones(n, dtype=bool)
        others[u] = False
        for v in nb:
            others[v] = False
            with np.errstate(all="ignore"):
                below.append(int(np.count_nonzero(d[others] < d[v])))
                equal.append(int(np.count_nonzero(d[others] == d[v])))
            others[v] = True
        nbrs.append(nb)
        d2s.append(d[nb])
    return {"sources": rows.copy(), "indptr": indptr,
            "neighbors": np.concatenate(nbrs).astype(np.int32) if nbrs else np.zeros(0, dtype=np.int32),
            "dist2": np.concatenate(d2s).astype(np.float32) if d2s else np.zeros(0, dtype=np.float32),
            "below": np.asarray(below, dtype=np.int64), "equal": np.asarray(equal, dtype=np.int64)}


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the metrics, by brute force from their definitions -------------------------------------------------------------------
def link_auc(pos, edges, rows=None):
    """P(a neighbour is nearer than a non-neighbour), ties one half, pooled over the sources with k_u >= 1 and m_u >= 1: a
    direct count over all (neighbour, non-neighbour) pairs per source, in doubled units so that it stays an integer."""
    pos = np.asarray(pos, dtype=np.float32)
    n = len(pos)
    gp, gi = simple_graph(n, edges)
    rows = range(n) if rows is None else [int(u) for u in np.asarray(rows).ravel()]
    num = den = 0
    for u in rows:
        nb = gi[gp[u]:gp[u + 1]]
        non = np.ones(n, dtype=bool)
        non[u] = False
        non[nb] = False
        k, m = len(nb), int(non.sum())
        if k < 1 or m < 1:
            continue
        d = dist2_from(pos, u)
        dn = d[non]
        for v in nb:
            with np.errstate(all="ignore"):
                nearer, tied = int(np.count_nonzero(dn < d[v])), int(np.count_nonzero(dn == d[v]))
            num += 2 * (m - nearer - tied) + tied   # a non-neighbour neither nearer nor tied is farther (NaN included)
        den += 2 * k * m
    return num / den if den else math.nan


def neighborhood_preservation(pos, edges, rows=None):
    """(precision, jaccard) by a direct sort per source: h_u = the neighbours among the k_u nearest other vertices, where a
    vertex as near as a neighbour never displaces it (ties count in the neighbour's favour): v is in iff fewer than k_u
    other vertices are strictly nearer."""
    pos = np.asarray(pos, dtype=np.float32)
    n = len(pos)
    gp, gi = simple_graph(n, edges)
    rows = range(n) if rows is None else [int(u) for u in np.asarray(rows).ravel()]
    hs, ks, jac = 0, 0, []
    for u in rows:
        nb = gi[gp[u]:gp[u + 1]]
        k = len(nb)
        if k < 1:
            continue
        d = dist2_from(pos, u)
        rest = np.sort(np.delete(d, u))          # NaN sorts last: it is below nothing
        h = 0
        for v in nb:
            # the sorted position of the first value not below d(u, v) = how many are strictly nearer; nothing is nearer
            # than a NaN distance under IEEE comparisons
            strictly_nearer = 0 if np.isnan(d[v]) else int(np.searchsorted(rest, d[v], side="left"))
            h += strictly_nearer < k
        hs += h
        ks += k
        jac.append(h / (2 * k - h))
    return (hs / ks if ks else math.nan), (math.fsum(jac) / len(jac) if jac else math.nan)
