"""The layout-quality rule of include/graphem_hip.h restated in numpy, for the tests: the crossing test on float32 arrays
(numpy rounds every operation to the array's type and contracts nothing), the per-edge counts, and the edge lengths with
math.fsum over Python doubles for the two sums.  dtype=np.float64 evaluates the same formula in double, which is NOT the
rule: the tests use it to show that a double-precision kernel would give other counts."""
import math

import numpy as np

ROW_CHUNK = 256


def orient(p, q, r):
    """(q0 - p0) * (r1 - p1) - (q1 - p1) * (r0 - p0) on arrays of points (..., 2), in the arrays' own type."""
    return (q[..., 0] - p[..., 0]) * (r[..., 1] - p[..., 1]) - (q[..., 1] - p[..., 1]) * (r[..., 0] - p[..., 0])


def _points(pos, edges, dtype):
    pos = np.asarray(pos, dtype=np.float32)
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    xy = pos[:, :2].astype(dtype)
    return edges, xy[edges[:, 0]], xy[edges[:, 1]]


def cross(a, b, c, d, ei, ej, dtype=np.float32):
    """The test for broadcastable arrays of segments (a, b) with vertex ids ei (..., 2) and (c, d) with ej."""
    zero = dtype(0)
    shared = ((ei[..., 0] == ej[..., 0]) | (ei[..., 0] == ej[..., 1]) | (ei[..., 1] == ej[..., 0]) | (ei[..., 1] == ej[..., 1]))
    with np.errstate(all="ignore"):
        first = orient(a, b, c) * orient(a, b, d) < zero
        second = orient(c, d, a) * orient(c, d, b) < zero
    return ~shared & first & second


def crossing_counts(pos, edges, rows=None, dtype=np.float32):
    """int64 counts[r] = the number of edges crossing edge rows[r] (None: every edge in order)."""
    pos = np.asarray(pos, dtype=np.float32)
    edges, a, b = _points(pos, edges, dtype) if pos.shape[1] >= 2 else (np.asarray(edges, dtype=np.int64).reshape(-1, 2), None, None)
    rows = np.arange(len(edges)) if rows is None else np.asarray(rows, dtype=np.int64).ravel()
    counts = np.zeros(len(rows), dtype=np.int64)
    if pos.shape[1] < 2 or len(edges) == 0:
        return counts
    for lo in range(0, len(rows), ROW_CHUNK):
        i = rows[lo:lo + ROW_CHUNK]
        m = cross(a[i][:, None], b[i][:, None], a[None], b[None], edges[i][:, None], edges[None], dtype)
        counts[lo:lo + ROW_CHUNK] = m.sum(axis=1)
    return counts


def pair_crossings(pos, edges, pairs, dtype=np.float32):
    """bool per pair (i, j) of edge ids."""
    pos = np.asarray(pos, dtype=np.float32)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if pos.shape[1] < 2 or len(pairs) == 0:
        return np.zeros(len(pairs), dtype=bool)
    edges, a, b = _points(pos, edges, dtype)
    i, j = pairs[:, 0], pairs[:, 1]
    return cross(a[i], b[i], a[j], b[j], edges[i], edges[j], dtype) & (i != j)


def edge_lengths(pos, edges):
    """float64 length of every edge: the squares of the double differences added in coordinate order, then sqrt."""
    pos = np.asarray(pos, dtype=np.float32).astype(np.float64)
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    s = np.zeros(len(edges))
    for d in range(pos.shape[1]):
        t = pos[edges[:, 0], d] - pos[edges[:, 1], d]
        s = s + t * t
    return np.sqrt(s)


def length_sums(pos, edges):
    """(min, max, sum L, sum L^2): the sums by math.fsum over Python doubles; (inf, -inf, 0, 0) without edges."""
    L = [float(v) for v in edge_lengths(pos, edges)]
    if not L:
        return math.inf, -math.inf, 0.0, 0.0
    return min(L), max(L), math.fsum(L), math.fsum(v * v for v in L)


def estimate(counts, E):
    """(estimate, standard error) of the crossing number from the counts of S sampled edges out of E."""
    S = len(counts)
    est = E / (2 * S) * int(np.sum(counts))
    if S == E or S < 2:
        return est, 0.0
    return est, E / 2 * np.std(np.asarray(counts, dtype=np.float64), ddof=1) / np.sqrt(S) * np.sqrt(1 - S / E)
