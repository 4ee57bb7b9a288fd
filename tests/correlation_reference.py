"""The rank-correlation rules of include/graphem_hip.h restated in integers, for the tests: the resample indices, the
multiplicities, u from the tie groups of a column (found with np.unique, no sort order involved), and the three sums of
a pair as Python integers.  Slow and plain on purpose."""
import math

import numpy as np

MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def word(seed, i, j):
    return mix(mix((seed + (i + 1) * GOLDEN) & MASK) ^ j)


def _mix_array(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def resample_indices(n, b, seed):
    """idx(b, j) = floor(word(seed, b, j) * n / 2^64) for j = 0 .. n-1, int64.  Vectorised; n < 2^21, so with
    word = hi * 2^32 + lo the quotient is (hi * n + (lo * n >> 32)) >> 32 without leaving 64 bits.  The first and last
    entries are checked against the scalar form."""
    stream = np.uint64(mix((seed + (b + 1) * GOLDEN) & MASK))
    with np.errstate(over="ignore"):
        w = _mix_array(stream ^ np.arange(n, dtype=np.uint64))
    hi, lo = w >> np.uint64(32), w & np.uint64(0xFFFFFFFF)
    idx = ((hi * np.uint64(n) + ((lo * np.uint64(n)) >> np.uint64(32))) >> np.uint64(32)).astype(np.int64)
    for j in (0, n - 1):
        assert int(idx[j]) == (word(seed, b, j) * n) >> 64
    return idx


def multiplicities(n, b, seed):
    return np.bincount(resample_indices(n, b, seed), minlength=n).astype(np.int64)


def u_values(column, c):
    """u_i = 2 B_g(i) + C_g(i) - n, groups = equal values of the column (-0.0 == 0.0), ascending."""
    column = np.asarray(column, dtype=np.float64)
    n = int(np.sum(c))
    _, group = np.unique(column, return_inverse=True)     # equal values (by ==) share a group, groups ascend
    C = np.zeros(group.max() + 1, dtype=np.int64)
    np.add.at(C, group, c)
    B = np.cumsum(C) - C
    return (2 * B + C - n)[group]


def triples(columns, pairs, c):
    """[(Sxy, Sxx, Syy)] as Python integers for every pair (x, y) of column ids, all under the weights c."""
    w = [int(a) for a in c]
    u = {col: [int(a) for a in u_values(columns[col], c)] for col in {int(q) for pair in pairs for q in pair}}
    return [(sum(k * a * b for k, a, b in zip(w, u[x], u[y])), sum(k * a * a for k, a in zip(w, u[x])),
             sum(k * b * b for k, b in zip(w, u[y]))) for x, y in pairs]


def triple(x, y, c):
    return triples([x, y], [(0, 1)], c)[0]


def rho_of(sxy, sxx, syy):
    if sxx == 0 or syy == 0:
        return math.nan
    return float(sxy) / math.sqrt(float(sxx) * float(syy))


def plain_triple(x, y):
    return triple(x, y, np.ones(len(x), dtype=np.int64))


def bootstrap_triple(x, y, b, seed):
    return triple(x, y, multiplicities(len(x), b, seed))
