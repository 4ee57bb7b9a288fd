"""The Lanczos operators and one step of gh_trlan_sweep (csrc/spectral.hip), restated in numpy at extended precision, and
the checker that holds a float64 implementation to them stage by stage.  TEST INFRASTRUCTURE ONLY.

Thick-restart Lanczos with full reorthogonalisation corrects itself: a wrong coefficient or a dot product that misses a
chunk costs steps and the eigenpairs still come out, so a converged solve says little about the kernels.  Here every stage
of a step is evaluated in np.longdouble FROM THE IMPLEMENTATION'S OWN previous-stage outputs (all float64 arrays), so the
only difference left is that stage's rounding, and every bar is a textbook forward-error bound computed from the data
(Higham, Accuracy and Stability of Numerical Algorithms, ch. 3): with u = 2^-53 and gamma_k = k u / (1 - k u), a sum of k
products in any order is within gamma_k sum |terms| of the exact one.  The bars carry a leading factor 2, which absorbs
this module's own rounding (x87 80-bit: eps 1.08e-19).  Where long double is no wider than that (eps >= 2e-19: it is an
alias of double on some platforms) the module computes in float64 and says so once; the bars do not move.

One step j of a sweep over the basis rows V[0 .. R), R = nl + j + 1 (the first nl are locked vectors), v = V[R - 1]:
    w0 = B v                        B = 2I - L (symnorm below)
    h1 = V w0                       first classical Gram-Schmidt pass
    w1 = w0 - h1^T V                (never stored: the second pass overwrites it)
    h2 = V w1
    w2 = w1 - h2^T V                work[0 : n] after the step
    beta = |w2|,  Td[r - nl][j] = h1[r] + h2[r] for nl <= r < R,  hmax = max |Td[.][j]|,  V[R] = w2 / beta
"""
import numpy as np
import scipy.sparse as sp

LD = np.longdouble
if not np.finfo(np.longdouble).eps < 2e-19:
    LD = np.float64
    print("spectral_reference: np.longdouble is not an extended type here (eps %g): computing in float64"
          % np.finfo(np.longdouble).eps)

U = LD(2.0) ** -53


def _ld(a):
    return np.asarray(a, dtype=LD)


def gamma(k):
    """gamma_k = k u / (1 - k u), long double; k a number or an integer array."""
    ku = _ld(k) * U
    return ku / (LD(1.0) - ku)


def row_sums(indptr, vals):
    """sum of vals over every CSR row (long double), 0 for an empty row."""
    indptr = np.asarray(indptr, dtype=np.int64)
    out = np.zeros(len(indptr) - 1, dtype=LD)
    filled = np.diff(indptr) > 0
    if filled.any():                     # (reduceat takes an empty segment for a one-element one: leave them out)
        out[filled] = np.add.reduceat(_ld(vals), indptr[:-1][filled])
    return out


def symnorm(indptr, indices, s, x):
    """(y, yabs): y_i = x_i + s_i sum_j s_j x_j over the neighbours j of i, y_i = 2 x_i for an isolated vertex, from the
    float64 s = degree^-1/2 that spectral.py builds (0 for an isolated vertex); yabs the same expression over absolute
    values.  Both long double."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    s, x = _ld(s), _ld(x)
    isolated = np.diff(indptr) == 0
    sx = s * x
    y = x + s * row_sums(indptr, sx[indices])
    yabs = np.abs(x) + s * row_sums(indptr, np.abs(sx)[indices])
    y[isolated] = LD(2.0) * x[isolated]
    yabs[isolated] = LD(2.0) * np.abs(x[isolated])
    return y, yabs


def adj_shift(indptr, indices, c, x):
    """(y, yabs): y = A x + c x for the 0/1 adjacency A, and |A| |x| + |c| |x|.  Both long double."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    x = _ld(x)
    y = row_sums(indptr, x[indices]) + LD(c) * x
    yabs = row_sums(indptr, np.abs(x)[indices]) + abs(LD(c)) * np.abs(x)
    return y, yabs


def inv_sqrt_degree(indptr):
    """s as spectral.py builds it: float64 1 / sqrt(degree), 0 for an isolated vertex."""
    deg = np.diff(np.asarray(indptr)).astype(np.float64)
    return np.where(deg > 0, 1.0 / np.sqrt(np.maximum(deg, 1.0)), 0.0)


def _ratio(err, bound):
    """max err / bound (0 / 0 = 0, x / 0 = inf, NaN = inf) as a float."""
    err, bound = np.atleast_1d(_ld(err)), np.atleast_1d(_ld(bound))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, LD(0.0), err / bound)
    r = np.where(np.isnan(r), LD(np.inf), r)
    return float(r.max()) if r.size else 0.0


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def spmv_ratio(y_dev, y, yabs, indptr):
    """Largest |y_dev - y| / (2 gamma_{deg_i + 4} yabs_i): the per-row sum has deg_i products and at most deg_i + 3
    further roundings however its terms are grouped."""
    deg = np.diff(np.asarray(indptr, dtype=np.int64))
    return _ratio(np.abs(_ld(y_dev) - y), LD(2.0) * gamma(deg + 4) * yabs)


class StageError(AssertionError):
    """Raised by check_step: .stages names every stage out of its bound, .ratios has all of them."""

    def __init__(self, stages, ratios):
        super().__init__("stages outside their bound: %s (error / bound: %s)" % (
            ", ".join(stages), ", ".join("%s %.3g" % kv for kv in ratios.items())))
        self.stages, self.ratios = stages, ratios


def check_step(indptr, indices, s, V, nl, w0, h1, h2, w2, beta, hmax, tcol, vnext):
    """One step of the sweep, every stage against long double on the implementation's own earlier outputs (float64):
    V (R, n) the basis rows, v = V[R - 1]; w0 (n,); h1, h2 (R,); w2 (n,); beta, hmax scalars; tcol (R - nl,) = column j of
    Td; vnext (n,).  Returns {stage: largest error / bound}; raises StageError when one exceeds 1 or an exact stage
    differs in a bit."""
    V64 = np.ascontiguousarray(V, dtype=np.float64)
    R, n = V64.shape
    Vl, aV = _ld(V64), np.abs(_ld(V64))
    w0l, h1l, h2l, w2l = _ld(w0), _ld(h1), _ld(h2), _ld(w2)
    ratios, bad = {}, []

    def stage(name, ratio, ok=True):
        ratios[name] = ratio
        if not (ratio <= 1.0 and ok):
            bad.append(name)

    # w0 against the operator; an isolated row is 2 v_i exactly
    y, yabs = symnorm(indptr, indices, s, V64[R - 1])
    isolated = np.diff(np.asarray(indptr, dtype=np.int64)) == 0
    stage("w0", spmv_ratio(w0, y, yabs, indptr),
          same_bits(np.asarray(w0, dtype=np.float64)[isolated], 2.0 * V64[R - 1][isolated]))
    # h1 against V w0
    g_n = LD(2.0) * gamma(n + 2)
    g_r = LD(2.0) * gamma(R + 2)
    stage("h1", _ratio(np.abs(h1l - Vl @ w0l), g_n * (aV @ np.abs(w0l))))
    # w1 in long double only, with the uncertainty a float64 w1 carries
    w1 = w0l - h1l @ Vl
    e1 = g_r * (np.abs(w0l) + np.abs(h1l) @ aV)
    # h2 against V w1
    stage("h2", _ratio(np.abs(h2l - Vl @ w1), g_n * (aV @ np.abs(w1)) + aV @ e1))
    # w2 against w1 - h2^T V
    stage("w2", _ratio(np.abs(w2l - (w1 - h2l @ Vl)), e1 + g_r * (np.abs(w1) + np.abs(h2l) @ aV)))
    # beta against the norm of the implementation's w2
    norm = np.sqrt((w2l * w2l).sum())
    stage("beta", _ratio(abs(LD(beta) - norm), LD(2.0) * gamma(n + 3) * norm))
    # the projected column and its largest entry: float64 sums, bit for bit
    col = (np.asarray(h1, dtype=np.float64) + np.asarray(h2, dtype=np.float64))[nl:]
    stage("Td", 0.0, same_bits(tcol, col))
    stage("hmax", 0.0, same_bits(np.float64(hmax), np.abs(col).max()))
    # the next basis vector: w2 / beta within one ulp (IEEE division gives half; one allows a reciprocal sequence)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.asarray(w2, dtype=np.float64) / np.float64(beta)
        stage("vnext", _ratio(np.abs(np.asarray(vnext, dtype=np.float64) - q), np.spacing(np.abs(q))))
    if bad:
        raise StageError(bad, ratios)
    return ratios


# ---- builders -------------------------------------------------------------------------------------------------------

MIXED_DEGREES = (2, 7, 8, 9, 15, 16, 17, 63, 64, 65)


def mixed_degree_graph(n, seed=0):
    """(indptr int64, indices int32) of a symmetric 0/1 CSR with sorted rows and no diagonal on n vertices: one hub
    adjacent to every vertex that has an edge at all; for each degree d of MIXED_DEGREES, as long as it fits, a group of
    vertices of exactly that degree (the hub plus a circulant of degree d - 1 inside the group); of the rest about a
    quarter isolated (at least one from n = 3 on) and the others leaves on the hub.  Vertex ids are shuffled, so the
    degrees are scattered over the workgroups.  n = 1: one isolated vertex; n = 2: one edge."""
    rng = np.random.default_rng(seed)
    if n == 1:
        return np.zeros(2, dtype=np.int64), np.zeros(0, dtype=np.int32)
    rows, cols = [], []
    nxt = 1                                            # vertex 0 is the hub
    n_isolated = 0 if n < 3 else max(1, (n - 1) // 16)
    room = n - 1 - n_isolated
    for d in MIXED_DEGREES:
        g = d + 1 + ((d + 1) & 1)                      # even, and larger than the inner degree d - 1
        if g > room - 1:                               # (keep one leaf)
            break
        v = np.arange(g)
        for off in range(1, (d - 1) // 2 + 1):
            rows.append(nxt + v)
            cols.append(nxt + (v + off) % g)
        if (d - 1) % 2:
            rows.append(nxt + v[: g // 2])
            cols.append(nxt + v[: g // 2] + g // 2)
        nxt += g
        room -= g
    nxt += room                                        # the leaves
    rows.append(np.zeros(nxt - 1, dtype=np.int64))
    cols.append(np.arange(1, nxt))
    r, c = np.concatenate(rows), np.concatenate(cols)
    perm = rng.permutation(n)
    r, c = perm[r], perm[c]
    a = sp.coo_matrix((np.ones(2 * len(r)), (np.concatenate([r, c]), np.concatenate([c, r]))), shape=(n, n)).tocsr()
    a.sum_duplicates()
    a.sort_indices()
    assert a.data.max() == 1.0 and a.diagonal().max() == 0.0
    return a.indptr.astype(np.int64), a.indices.astype(np.int32)


def edgeless_graph(n):
    return np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=np.int32)


def orthonormal_basis(R, n, seed=0):
    """(R, n) float64 with orthonormal rows: QR of a seeded normal matrix."""
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((n, R)))
    return np.ascontiguousarray(q.T)


def oblique_basis(R, n, seed=0):
    """(R, n) float64 unit rows with pairwise correlation near 0.3: a shared normal direction in every row.  Against it
    the second Gram-Schmidt pass carries real numbers, not rounding noise."""
    rng = np.random.default_rng(seed)
    rows = np.sqrt(0.3) * rng.standard_normal(n) + np.sqrt(0.7) * rng.standard_normal((R, n))
    return np.ascontiguousarray(rows / np.linalg.norm(rows, axis=1, keepdims=True))


def scaled_normal(n, seed=0):
    """normal x 10^uniform(-3, 3): entries of either sign over six decades."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) * 10.0 ** rng.uniform(-3.0, 3.0, n)
