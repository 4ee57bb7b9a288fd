"""The fp64 kernels of the spectral start, each against tests/spectral_reference.py: spmv_symnorm_kernel and the four
Gram-Schmidt kernels behind gh_trlan_sweep (csrc/spectral.hip), and spmv_adj_shift_kernel (csrc/centrality.hip).

A converged eigensolve hides an arithmetic slip in them (full reorthogonalisation corrects itself), so here one step of a
sweep is taken apart: w0, h1, h2 and w2 are read from the work buffer (its layout is part of the header's contract) and
every stage is held to a long-double evaluation of the same stage on the device's own earlier outputs.  Shapes: basis
heights below, at and above the kernels' groups of 16 rows up to the 255 the staging allows, locked rows, vector lengths
around the 512-element chunk and one with more than 256 chunks (the second trip of the strided reduce loops); degrees 0,
1, 7, 8, 9 ... around the 8 lanes of a row, a hub row and a last partial workgroup for the SpMVs.

Every output buffer is at least 64 doubles longer than the header asks for; the excess, and every entry a call has no
business writing, holds a sentinel that must still be there afterwards.
"""
import ctypes

import numpy as np
import pytest

import spectral_reference as ref

pytestmark = pytest.mark.gpu

SENTINEL = -6.02214076e123
PAD = 64
GH_OK, GH_ERR_INVALID = 0, 1
DEV = "cuda:0"


def _show(what, ratios):
    """The error / bound ratios of a case, for the record (pytest -s): information, not a criterion."""
    print(f"\n{what}: " + ", ".join(f"{k} {v:.2e}" for k, v in ratios.items()))


def _torch():
    import torch
    return torch


def _lib():
    from graphem_rapids_amd import _native
    return _native.load()


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(_torch().cuda.current_stream(DEV).cuda_stream)


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).to(DEV)


def _padded(values, size=None):
    """A device float64 buffer of `size` (default: len(values)) + PAD doubles: values first, the sentinel after."""
    values = np.asarray(values, dtype=np.float64).ravel()
    size = len(values) if size is None else size
    host = np.full(size + PAD, SENTINEL)
    host[: len(values)] = values
    return _dev(host)


def _host(t):
    _torch().cuda.synchronize()
    return t.cpu().numpy()


def _untouched(a):
    return bool(np.all(np.asarray(a) == SENTINEL))


class Graph:
    """A CSR on the device as spectral.py uploads it."""

    def __init__(self, indptr, indices):
        self.indptr, self.indices = indptr, indices
        self.n = len(indptr) - 1
        self.s = ref.inv_sqrt_degree(indptr)
        self.d_indptr = _dev(indptr.astype(np.int64))
        # (a zero-size tensor has a null data_ptr, which the entry points reject: one padding element)
        self.d_indices = _dev(indices.astype(np.int32) if len(indices) else np.zeros(1, dtype=np.int32))
        self.d_s = _dev(self.s)

    def spmv(self, x):
        """gh_spmv_symnorm on a host vector: (y (n,), the sentinel tail)."""
        d_x, d_y = _dev(np.asarray(x, dtype=np.float64)), _padded([], self.n)
        st = _lib().gh_spmv_symnorm(_stream(), self.n, _vp(self.d_indptr), _vp(self.d_indices), _vp(self.d_s), _vp(d_x),
                                    _vp(d_y))
        assert st == GH_OK, _lib().gh_spectral_last_error()
        y = _host(d_y)
        return y[: self.n], y[self.n:]

    def sweep(self, d_V, nl, m, k, d_Td, d_work, d_beta, d_hmax, n=None):
        return _lib().gh_trlan_sweep(_stream(), self.n if n is None else n, _vp(self.d_indptr), _vp(self.d_indices),
                                     _vp(self.d_s), _vp(d_V), int(nl), int(m), int(k), _vp(d_Td), _vp(d_work), _vp(d_beta),
                                     _vp(d_hmax))


_GRAPHS = {}


def _graph(n):
    if n not in _GRAPHS:
        _GRAPHS[n] = Graph(*ref.mixed_degree_graph(n, seed=n))
    return _GRAPHS[n]


def _work_size(n, nl, m):
    return n + 2 * (nl + m + 1) + ((n + 511) // 512) * (nl + m + 1)


# ---- the two SpMVs ---------------------------------------------------------------------------------------------------

SPMV_SIZES = [1, 2, 31, 32, 33, 257, 1000, 4099]


def _spmv_graph(n):
    return Graph(*ref.edgeless_graph(5)) if n == "edgeless" else _graph(n)


@pytest.mark.parametrize("n", SPMV_SIZES + ["edgeless"])
def test_spmv_symnorm_rows(n):
    g = _spmv_graph(n)
    x = ref.scaled_normal(g.n, seed=g.n + 7)
    y, tail = g.spmv(x)
    y_again, _ = g.spmv(x)
    assert _untouched(tail)
    assert ref.same_bits(y, y_again)
    want, wabs = ref.symnorm(g.indptr, g.indices, g.s, x)
    ratio = ref.spmv_ratio(y, want, wabs, g.indptr)
    _show(f"gh_spmv_symnorm n = {g.n}", {"y": ratio})
    assert ratio <= 1.0, ratio
    isolated = np.diff(g.indptr) == 0
    assert ref.same_bits(y[isolated], 2.0 * x[isolated])


@pytest.mark.parametrize("n", SPMV_SIZES + ["edgeless"])
def test_spmv_adj_shift_rows(n):
    torch = _torch()
    from graphem_rapids_amd import _native
    from graphem_rapids_amd.embedder_hip import device_view
    if n == "edgeless":
        n, indptr, indices = 5, *ref.edgeless_graph(5)
    else:
        indptr, indices = ref.mixed_degree_graph(n, seed=n)
    rows = np.repeat(np.arange(n), np.diff(indptr))
    upper = np.stack([rows, indices], axis=1)[rows < indices].astype(np.int32)
    # the handle symmetrises and drops duplicates and self-loops: give it some of each
    edges = np.concatenate([upper, upper[::3, ::-1], upper[:5], np.array([[0, 0], [n - 1, n - 1]], dtype=np.int32)])
    cg = _native.CentGraph(n, edges)
    try:
        assert cg.edges == len(upper)
        ip, ix = cg.csr_device()
        h_indptr = device_view(ip, (n + 1,), torch.int64, torch.device(DEV), cg).cpu().numpy()
        nnz = int(h_indptr[-1])
        h_indices = (device_view(ix, (nnz,), torch.int32, torch.device(DEV), cg).cpu().numpy() if nnz
                     else np.zeros(0, dtype=np.int32))
        assert np.array_equal(h_indptr, indptr) and np.array_equal(h_indices, indices)
        x = ref.scaled_normal(n, seed=n + 11)
        d_x = _dev(x)
        for c in (0.0, 1.0, -2.5):
            out = []
            for _ in range(2):
                d_y = _padded([], n)
                cg.spmv_shift(torch.cuda.current_stream(DEV).cuda_stream, d_x.data_ptr(), d_y.data_ptr(), c)
                out.append(_host(d_y))
            assert _untouched(out[0][n:])
            assert ref.same_bits(out[0], out[1])
            want, wabs = ref.adj_shift(h_indptr, h_indices, c, x)
            ratio = ref.spmv_ratio(out[0][:n], want, wabs, h_indptr)
            _show(f"gh_spmv_adj_shift n = {n}, c = {c}", {"y": ratio})
            assert ratio <= 1.0, (c, ratio)
    finally:
        cg.close()


# ---- one step of the sweep -------------------------------------------------------------------------------------------

def _one_step(g, V_rows, nl, j, spare_rows=1):
    """Step j alone (k = j, m = j + 1) on the basis rows V_rows (R = nl + j + 1 of them): everything the call left behind,
    as host arrays, after the sentinels around it were checked."""
    n, m, R = g.n, j + 1, nl + j + 1
    assert V_rows.shape == (R, n)
    rows = R + 1 + spare_rows                     # the header's nl + m + 1 rows, then rows no step may reach
    d_V = _padded(V_rows, rows * n)
    d_Td, d_beta, d_hmax = _padded([], m * m), _padded([], m), _padded([], m)
    wsize = _work_size(n, nl, m)
    d_work = _padded([], wsize)
    st = g.sweep(d_V, nl, m, j, d_Td, d_work, d_beta, d_hmax)
    assert st == GH_OK, _lib().gh_spectral_last_error()
    V, Td, beta, hmax, work = (_host(t) for t in (d_V, d_Td, d_beta, d_hmax, d_work))
    assert ref.same_bits(V[: R * n].reshape(R, n), V_rows)                       # the basis is read, never written
    assert _untouched(V[(R + 1) * n:])
    assert _untouched(work[wsize:])
    assert _untouched(Td[m * m:]) and _untouched(beta[m:]) and _untouched(hmax[m:])
    Tdm = Td[: m * m].reshape(m, m)
    assert _untouched(Tdm[:, :j]) and _untouched(beta[:j]) and _untouched(hmax[:j])
    Rmax = nl + m + 1                                              # the documented layout of work: w, h1, h2, partials
    return dict(h1=work[n: n + R].copy(), h2=work[n + Rmax: n + Rmax + R].copy(), w2=work[:n].copy(), beta=beta[j],
                hmax=hmax[j], tcol=Tdm[:, j].copy(), vnext=V[R * n: (R + 1) * n].copy())


def _same_step(a, b):
    return all(ref.same_bits(a[key], b[key]) for key in a)


SWEEP_CASES = [(300, 0, 0), (511, 0, 14), (512, 0, 15), (513, 3, 13), (1000, 16, 16), (257, 0, 4), (600, 100, 154),
               (700, 254, 0), (140000, 2, 3)]                      # (n, nl, j); R = nl + j + 1


# both bases, except that R = 255 runs with the orthonormal one only
SWEEP_PARAMS = [c + (b,) for c in SWEEP_CASES for b in ("orthonormal", "oblique") if b == "orthonormal" or c[1] + c[2] + 1 < 255]


@pytest.mark.parametrize("n,nl,j,basis", SWEEP_PARAMS)
def test_one_sweep_step_stage_by_stage(n, nl, j, basis):
    R = nl + j + 1
    g = _graph(n)
    V = (ref.orthonormal_basis if basis == "orthonormal" else ref.oblique_basis)(R, n, seed=R)
    out = _one_step(g, V, nl, j)
    assert _same_step(out, _one_step(g, V, nl, j))                 # fixed summation order: bit-identical runs
    w0, _ = g.spmv(V[R - 1])                                       # the same launch as the sweep's first
    ratios = ref.check_step(g.indptr, g.indices, g.s, V, nl, w0=w0, **out)
    _show(f"sweep step (n, nl, j) = ({n}, {nl}, {j}), {basis}", ratios)


# ---- several steps ---------------------------------------------------------------------------------------------------

def test_a_sweep_is_the_chain_of_its_steps():
    """k = 3 .. m = 12 in one call against nine single-step calls: the same launches in the same order, so V, the Td
    columns, beta and hmax agree bit for bit; every step of the chain also goes through the stage checker.  Td columns
    below k, the lower triangle and every buffer's excess keep their sentinel."""
    n, nl, k, m = 1000, 4, 3, 12
    g = _graph(n)
    start = ref.orthonormal_basis(nl + k + 1, n, seed=99)
    rows = nl + m + 1
    d_V = _padded(start, rows * n)
    d_Td, d_beta, d_hmax = _padded([], m * m), _padded([], m), _padded([], m)
    wsize = _work_size(n, nl, m)
    d_work = _padded([], wsize)
    assert g.sweep(d_V, nl, m, k, d_Td, d_work, d_beta, d_hmax) == GH_OK
    V, Td, beta, hmax, work = (_host(t) for t in (d_V, d_Td, d_beta, d_hmax, d_work))
    assert _untouched(V[rows * n:]) and _untouched(work[wsize:])
    assert _untouched(Td[m * m:]) and _untouched(beta[m:]) and _untouched(hmax[m:])
    assert _untouched(beta[:k]) and _untouched(hmax[:k])
    V, Td = V[: rows * n].reshape(rows, n), Td[: m * m].reshape(m, m)
    assert ref.same_bits(V[: nl + k + 1], start)
    assert _untouched(Td[:, :k])
    assert _untouched(Td[np.tril_indices(m, -1)])
    chain = start
    for j in range(k, m):
        R = nl + j + 1
        out = _one_step(g, chain, nl, j)
        w0, _ = g.spmv(chain[R - 1])
        _show(f"chain step {j}", ref.check_step(g.indptr, g.indices, g.s, chain, nl, w0=w0, **out))
        assert ref.same_bits(Td[: j + 1, j], out["tcol"]), j
        assert ref.same_bits(beta[j], out["beta"]) and ref.same_bits(hmax[j], out["hmax"]), j
        assert ref.same_bits(V[R], out["vnext"]), j
        chain = np.vstack([chain, out["vnext"][None, :]])


# ---- remaining cases -------------------------------------------------------------------------------------------------

def test_an_empty_sweep_writes_nothing():
    n, nl, m = 300, 2, 5
    g = _graph(n)
    bufs = [_padded([], (nl + m + 1) * n), _padded([], m * m), _padded([], _work_size(n, nl, m)), _padded([], m),
            _padded([], m)]
    d_V, d_Td, d_work, d_beta, d_hmax = bufs
    assert g.sweep(d_V, nl, m, m, d_Td, d_work, d_beta, d_hmax) == GH_OK
    for t in bufs:
        assert _untouched(_host(t))


def test_invariant_subspace_leaves_a_tiny_beta():
    """B = 2I on an edgeless graph: w0 = 2 v exactly, so after the two passes only rounding is left and the step meets the
    caller's own exhaustion rule (spectral.py: beta < 1e-13 max(1, hmax))."""
    n = 600
    g = Graph(*ref.edgeless_graph(n))
    v = ref.orthonormal_basis(1, n, seed=6)
    d_V = _padded(v, 2 * n)
    d_Td, d_beta, d_hmax, d_work = _padded([], 1), _padded([], 1), _padded([], 1), _padded([], _work_size(n, 0, 1))
    assert g.sweep(d_V, 0, 1, 0, d_Td, d_work, d_beta, d_hmax) == GH_OK
    beta, hmax, Td = _host(d_beta), _host(d_hmax), _host(d_Td)
    assert _untouched(beta[1:]) and _untouched(hmax[1:]) and _untouched(Td[1:])
    assert abs(Td[0] - 2.0) <= 1e-14 and hmax[0] == abs(Td[0])
    assert 0.0 <= beta[0] < 1e-13 * max(1.0, hmax[0]), (beta[0], hmax[0])


def test_argument_checks():
    """Host-side: nothing is launched, every buffer keeps its sentinel."""
    lib = _lib()
    n = 300
    g = _graph(n)

    def bufs(rows, m):
        return [_padded([], rows * n), _padded([], m * m), _padded([], _work_size(n, 0, rows)), _padded([], m), _padded([], m)]

    def rejected(call):
        st = call()
        assert st == GH_ERR_INVALID, st
        assert b"bad argument" in lib.gh_spectral_last_error()

    b = bufs(257, 200)
    d_V, d_Td, d_work, d_beta, d_hmax = b
    rejected(lambda: g.sweep(d_V, 56, 200, 0, d_Td, d_work, d_beta, d_hmax))       # nl + m + 1 == 257
    rejected(lambda: g.sweep(d_V, 0, 5, 6, d_Td, d_work, d_beta, d_hmax))          # k > m
    rejected(lambda: g.sweep(d_V, -1, 5, 0, d_Td, d_work, d_beta, d_hmax))         # nl < 0
    rejected(lambda: g.sweep(d_V, 0, 5, 0, d_Td, d_work, d_beta, d_hmax, n=0))     # n == 0
    rejected(lambda: lib.gh_trlan_sweep(_stream(), n, _vp(g.d_indptr), _vp(g.d_indices), _vp(g.d_s), None, 0, 5, 0,
                                        _vp(d_Td), _vp(d_work), _vp(d_beta), _vp(d_hmax)))     # a null pointer
    rejected(lambda: lib.gh_spmv_symnorm(_stream(), n, _vp(g.d_indptr), _vp(g.d_indices), _vp(g.d_s), None, _vp(d_work)))
    for t in b:
        assert _untouched(_host(t))

