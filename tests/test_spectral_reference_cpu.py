"""Anchors tests/spectral_reference.py -- the extended-precision Lanczos step the kernels of csrc/spectral.hip and the
adjacency SpMV of csrc/centrality.hip are compared with in tests/test_hip_spectral_kernels.py -- without a GPU:
  * its operator is scipy's normalised Laplacian: B = 2I - csgraph.laplacian(sym, normed=True);
  * a float64 numpy stand-in for the device (chunked sums of 512, row-by-row updates) passes every stage of the checker;
  * the same stand-in with one small arithmetic slip is rejected, at the stage the slip belongs to.
"""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import laplacian

import spectral_reference as ref

CHUNK = 512
SHAPES = [(257, 255), (513, 17), (1000, 16), (3000, 33), (20000, 5)]      # (n, R)


def test_builder_has_the_promised_degrees():
    indptr, indices = ref.mixed_degree_graph(1000, seed=1)
    n = len(indptr) - 1
    deg = np.diff(indptr)
    a = sp.csr_matrix((np.ones(len(indices)), indices, indptr), shape=(n, n))
    assert (a != a.T).nnz == 0 and a.diagonal().max() == 0
    for d in (0, 1) + ref.MIXED_DEGREES:
        assert (deg == d).any(), d
    hub = int(np.argmax(deg))
    assert deg[hub] == (deg > 0).sum() - 1             # adjacent to every other vertex that has an edge
    for small in (1, 2, 3, 31, 32, 33, 257):
        ip, ix = ref.mixed_degree_graph(small, seed=small)
        assert len(ip) == small + 1 and ip[-1] == len(ix) and (ix < small).all()
    assert np.diff(ref.mixed_degree_graph(2)[0]).tolist() == [1, 1]
    assert (np.diff(ref.mixed_degree_graph(33, seed=4)[0]) == 0).any()


@pytest.mark.parametrize("n", [2, 33, 257, 1000])
def test_operator_is_two_minus_scipys_normalised_laplacian(n):
    indptr, indices = ref.mixed_degree_graph(n, seed=n)
    a = sp.csr_matrix((np.ones(len(indices)), indices, indptr), shape=(n, n))
    B = 2.0 * np.eye(n) - laplacian(a, normed=True).toarray()
    x = ref.scaled_normal(n, seed=n + 1)
    y, yabs = ref.symnorm(indptr, indices, ref.inv_sqrt_degree(indptr), x)
    # scipy's entries are 1 / sqrt(d_i) / sqrt(d_j): within 7 u of the product of the float64 s_i and s_j, then one
    # product and at most deg additions per row -- deg + 8 roundings against the bar's 2 (deg + 4)
    assert ref.spmv_ratio(B @ x, y, yabs, indptr) <= 1.0
    assert ref.same_bits(y[np.diff(indptr) == 0].astype(np.float64), 2.0 * x[np.diff(indptr) == 0])


def test_adjacency_operator_matches_scipy():
    n = 257
    indptr, indices = ref.mixed_degree_graph(n, seed=3)
    a = sp.csr_matrix((np.ones(len(indices)), indices, indptr), shape=(n, n))
    x = ref.scaled_normal(n, seed=4)
    for c in (0.0, 1.0, -2.5):
        y, yabs = ref.adj_shift(indptr, indices, c, x)
        assert ref.spmv_ratio(a @ x + c * x, y, yabs, indptr) <= 1.0


# ---- a float64 stand-in for the device --------------------------------------------------------------------------------

def _chunk_sums(terms):
    """Sum the last axis in chunks of 512, then the chunk sums: float64 throughout."""
    n = terms.shape[-1]
    starts = np.arange(0, n, CHUNK)
    return np.add.reduceat(terms, starts, axis=-1).sum(axis=-1)


def _spmv(indptr, indices, s, x, drop=None):
    n = len(indptr) - 1
    y = np.empty(n)
    for i in range(n):
        nb = indices[indptr[i]: indptr[i + 1]]
        if drop is not None and i == drop:
            nb = nb[:-1]
        y[i] = x[i] + s[i] * np.sum(s[nb] * x[nb]) if indptr[i + 1] > indptr[i] else 2.0 * x[i]
    return y


def standin_step(indptr, indices, s, V, nl, mutant=None):
    """What one step of the sweep leaves behind, computed in float64: the arguments of ref.check_step after V and nl."""
    R, n = V.shape
    drop = None
    if mutant == "spmv":
        drop = int(np.flatnonzero(np.diff(indptr) == 9)[0])
    w0 = _spmv(indptr, indices, s, V[R - 1], drop)
    terms = V * w0
    if mutant == "h1":
        terms[R // 2, n // 3] = 0.0
    h1 = _chunk_sums(terms)
    w = w0.copy()
    for r in range(R):
        w -= h1[r] * V[r]
    h2 = _chunk_sums(V * w)
    for r in range(R):
        w -= h2[r] * V[r]
    sq = w * w
    if mutant == "beta":
        sq = sq[: (n - 1) // CHUNK * CHUNK]
    beta = np.sqrt(_chunk_sums(sq))
    col = (h1 if mutant == "Td" else h1 + h2)[nl:]
    with np.errstate(divide="ignore", invalid="ignore"):      # (the beta mutant has nothing left at n <= 512)
        vnext = w / beta
    return dict(w0=w0, h1=h1, h2=h2, w2=w, beta=beta, hmax=np.abs(col).max(), tcol=col, vnext=vnext)


_GRAPHS = {}


def _case(n, R, basis):
    if n not in _GRAPHS:
        indptr, indices = ref.mixed_degree_graph(n, seed=n)
        _GRAPHS[n] = (indptr, indices, ref.inv_sqrt_degree(indptr))
    V = (ref.orthonormal_basis if basis == "orthonormal" else ref.oblique_basis)(R, n, seed=R)
    return _GRAPHS[n] + (V, min(3, R - 1))


def _bases(R):
    return ["orthonormal"] if R == 255 else ["orthonormal", "oblique"]


@pytest.mark.parametrize("n,R", SHAPES)
def test_standin_passes_every_stage(n, R):
    for basis in _bases(R):
        indptr, indices, s, V, nl = _case(n, R, basis)
        ratios = ref.check_step(indptr, indices, s, V, nl, **standin_step(indptr, indices, s, V, nl))
        print(n, R, basis, {k: "%.2e" % v for k, v in ratios.items()})
        assert set(ratios) == {"w0", "h1", "h2", "w2", "beta", "Td", "hmax", "vnext"}


@pytest.mark.parametrize("mutant,stage", [("h1", "h1"), ("beta", "beta"), ("Td", "Td"), ("spmv", "w0")])
@pytest.mark.parametrize("n,R", SHAPES)
def test_checker_rejects_a_slip(n, R, mutant, stage):
    """One term dropped from one h1; the last 512-chunk dropped from beta; h2 left out of Td; one neighbour dropped from
    one SpMV row of degree 9.  Each is rejected at its own stage, with either basis -- except that only the oblique basis
    shows the missing h2: against orthonormal rows h2 is rounding noise, which h1 + h2 may round away in every row."""
    for basis in ["oblique"] if mutant == "Td" else _bases(R):
        indptr, indices, s, V, nl = _case(n, R, basis)
        with pytest.raises(ref.StageError) as e:
            ref.check_step(indptr, indices, s, V, nl, **standin_step(indptr, indices, s, V, nl, mutant=mutant))
        assert stage in e.value.stages, (basis, e.value.stages)


def test_checker_rejects_a_wrong_isolated_row_and_a_two_ulp_quotient():
    indptr, indices, s, V, nl = _case(513, 17, "oblique")
    good = standin_step(indptr, indices, s, V, nl)
    iso = int(np.flatnonzero(np.diff(indptr) == 0)[0])
    out = dict(good, w0=good["w0"].copy())
    out["w0"][iso] = np.nextafter(out["w0"][iso], np.inf)
    with pytest.raises(ref.StageError) as e:
        ref.check_step(indptr, indices, s, V, nl, **out)
    assert "w0" in e.value.stages
    out = dict(good, vnext=good["vnext"].copy())
    out["vnext"][5] = np.nextafter(np.nextafter(out["vnext"][5], np.inf), np.inf)
    with pytest.raises(ref.StageError) as e:
        ref.check_step(indptr, indices, s, V, nl, **out)
    assert e.value.stages == ["vnext"]
    out = dict(good, hmax=np.nextafter(good["hmax"], np.inf))
    with pytest.raises(ref.StageError) as e:
        ref.check_step(indptr, indices, s, V, nl, **out)
    assert e.value.stages == ["hmax"]
