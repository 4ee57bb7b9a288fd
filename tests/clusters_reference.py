"""The clustering rule of include/graphem_hip.h ("embedding clusters") restated in numpy, for the tests.  The float32 chain is
written as separate numpy float32 operations in coordinate order (numpy rounds every operation to the array's type and
contracts nothing); the centre update adds int64 quantised coordinates with np.add.at; the distance sums are float64 sums per
row by math.fsum (the true sum to half an ulp).  Nothing of the package is imported."""
import math

import numpy as np


def dist2(pos, centres):
    """float32 (n, k): d2(x_v, centre_c) = (((0 + t_0 t_0) + t_1 t_1) + ...), t_d = x[v][d] - centre[c][d]."""
    pos, centres = np.asarray(pos, dtype=np.float32), np.asarray(centres, dtype=np.float32)
    s = np.zeros((len(pos), len(centres)), dtype=np.float32)
    with np.errstate(all="ignore"):
        for d in range(pos.shape[1]):
            t = pos[:, d, None] - centres[None, :, d]
            s = s + t * t
    assert s.dtype == np.float32
    return s


def assign(pos, centres):
    """(labels int32, d2 float32): c is walked upwards from best = +inf, label = 0 and taken when d2 < best, strictly -- the
    first index of the least distance, where a NaN or +inf distance is never taken."""
    d = dist2(pos, centres)
    d = np.where(np.isnan(d), np.float32(np.inf), d)
    labels = np.argmin(d, axis=1).astype(np.int32)   # the first of equal minima; 0 when every distance is +inf
    return labels, d[np.arange(len(d)), labels]


def shift_of(pos):
    """s = 38 - ilogb(M) for M = max |x|, 0 when M = 0."""
    m = float(np.max(np.abs(np.asarray(pos, dtype=np.float32)))) if np.size(pos) else 0.0
    return 38 - (math.frexp(m)[1] - 1) if m > 0 else 0


def update(pos, labels, centres):
    """The exact centre update: (centres float32 (k, D), counts int64)."""
    pos = np.asarray(pos, dtype=np.float32)
    k, D = centres.shape
    s = shift_of(pos)
    q = np.rint(np.ldexp(pos.astype(np.float64), s)).astype(np.int64)   # ties to even
    sums = np.zeros((k, D), dtype=np.int64)
    np.add.at(sums, labels, q)
    counts = np.bincount(labels, minlength=k).astype(np.int64)
    out = centres.copy()
    has = counts > 0
    out[has] = np.ldexp(sums[has].astype(np.float64) / counts[has, None].astype(np.float64), -s).astype(np.float32)
    return out, counts


def kmeans(pos, start, max_iter=300):
    """The Lloyd loop of the header.  dict: labels, centers, d2, counts, n_iter, converged."""
    pos = np.asarray(pos, dtype=np.float32)
    centres = np.array(start, dtype=np.float32)
    it, prev = 0, None
    while True:
        labels, d2 = assign(pos, centres)
        if it > 0 and np.array_equal(labels, prev):
            converged = True
            break
        if it == max_iter:
            converged = False
            break
        centres, _ = update(pos, labels, centres)
        prev = labels
        it += 1
    return {"labels": labels, "centers": centres, "d2": d2, "counts": np.bincount(labels, minlength=len(centres)).astype(np.int64),
            "n_iter": it, "converged": converged}


def min_d2_steps(pos, ids):
    """The running minimum after every seed step at ids[0], ids[1], ...: a list of float32 (n,) arrays."""
    pos = np.asarray(pos, dtype=np.float32)
    out, m = [], None
    for v in ids:
        d = dist2(pos, pos[v:v + 1])[:, 0]
        m = d if m is None else np.where(d < m, d, m)
        out.append(m)
    return out


def kmeans_plusplus(pos, k, seed=0):
    pos = np.asarray(pos, dtype=np.float32)
    n = len(pos)
    rng = np.random.default_rng(seed)
    ids = [int(rng.integers(n))]
    m = None
    while len(ids) < k:
        d = dist2(pos, pos[ids[-1]:ids[-1] + 1])[:, 0]
        m = d if m is None else np.where(d < m, d, m)
        cs = np.cumsum(m.astype(np.float64))
        if cs[-1] > 0:
            i = int(np.searchsorted(cs, rng.random() * cs[-1], side="right"))
            if i >= n:
                i = int(np.flatnonzero(m > 0)[-1])
        else:
            i = min(set(range(n)) - set(ids))
        ids.append(i)
    return np.array(ids, dtype=np.int64)


def distance_sums(pos, labels, k, rows=None):
    """float64 (len(rows), k): sums[r][c] = the sum over w with labels[w] == c, w != rows[r], of sqrt((double)d2(rows[r], w)),
    by math.fsum."""
    pos = np.asarray(pos, dtype=np.float32)
    n = len(pos)
    rows = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64).ravel()
    out = np.zeros((len(rows), k), dtype=np.float64)
    for r, u in enumerate(rows):
        d = np.sqrt(dist2(pos, pos[u:u + 1])[:, 0].astype(np.float64))
        keep = np.arange(n) != u
        for c in range(k):
            out[r, c] = math.fsum(d[keep & (labels == c)].tolist())
    return out


def terms(labels, k, rows=None):
    """int64 (len(rows), k): how many terms sums[r][c] has."""
    n = len(labels)
    rows = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64).ravel()
    counts = np.bincount(labels, minlength=k).astype(np.int64)
    out = np.tile(counts, (len(rows), 1))
    out[np.arange(len(rows)), labels[rows]] -= 1
    return out


def sums_close(got, want, n_terms):
    """The header's bound, on both sides of the comparison: each of two sums of N non-negative terms is within (N + 2) 2^-53
    of the true sum relatively, and the restatement's fsum within 2^-53; exactly 0 when N = 0."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and bool(np.all(np.abs(got - want) <= (n_terms + 3) * 2.0 ** -53 * np.abs(want)))


def silhouette(sums, labels, k, rows=None):
    """The silhouette from distance sums, one vertex at a time in Python floats."""
    n = len(labels)
    rows = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64).ravel()
    counts = np.bincount(labels, minlength=k)
    out = np.zeros(len(rows), dtype=np.float64)
    for r, u in enumerate(rows):
        own = int(labels[u])
        if counts[own] == 1:
            continue
        a = float(sums[r, own]) / (int(counts[own]) - 1)
        b = min(float(sums[r, c]) / int(counts[c]) for c in range(k) if c != own)
        out[r] = (b - a) / max(a, b) if max(a, b) > 0 else 0.0
    return out


def nmi(a, b):
    """Normalised mutual information with natural logarithms and the arithmetic mean, from Python integers."""
    a, b = list(np.asarray(a).ravel()), list(np.asarray(b).ravel())
    n = len(a)
    ca, cb, cab = {}, {}, {}
    for x, y in zip(a, b):
        ca[x] = ca.get(x, 0) + 1
        cb[y] = cb.get(y, 0) + 1
        cab[(x, y)] = cab.get((x, y), 0) + 1
    ha = math.fsum(c / n * math.log(n / c) for c in ca.values())
    hb = math.fsum(c / n * math.log(n / c) for c in cb.values())
    if ha == 0 and hb == 0:
        return 1.0
    mi = math.fsum(c / n * math.log(n * c / (ca[x] * cb[y])) for (x, y), c in cab.items())
    return mi / ((ha + hb) / 2)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
