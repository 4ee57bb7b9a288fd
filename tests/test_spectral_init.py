"""GPU spectral initialisation against the reference's method: scipy eigsh on the
normalised Laplacian (pt.py:337-379).  Eigenvectors are defined up to sign / rotation inside an
eigenspace, so eigenvalues and subspaces are compared."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla
from scipy.sparse.csgraph import laplacian

pytestmark = pytest.mark.gpu


def _reference_eig(adj, want):
    sym = sp.csr_matrix(adj + adj.transpose())
    sym.data = np.ones_like(sym.data)
    L = laplacian(sym, normed=True)
    vals, vecs = np.linalg.eigh(L.toarray())  # dense fp64: the exact answer eigsh approximates
    return L, vals[:want], vecs[:, :want]


@pytest.mark.parametrize("kind,n,D", [("rr", 600, 3), ("er", 800, 2), ("rr", 400, 16), ("grid", 400, 3), ("two", 300, 2)])
def test_eigenpairs_match_dense_reference(kind, n, D):
    import graphem_rapids_amd as gra
    from graphem_rapids_amd.spectral import laplacian_embedding_hip
    if kind == "rr":
        adj = gra.generate_random_regular(n, 6, seed=1)
    elif kind == "er":
        adj = gra.erdos_renyi_graph(n, 0.02, seed=2)       # has isolated vertices and small components
    elif kind == "grid":
        side = int(np.sqrt(n))
        idx = np.arange(side * side).reshape(side, side)
        e = np.vstack([np.column_stack([idx[:, :-1].ravel(), idx[:, 1:].ravel()]),
                       np.column_stack([idx[:-1, :].ravel(), idx[1:, :].ravel()])])
        adj = gra.edges_to_adjacency(side * side, e)       # degenerate eigenvalues (symmetry)
        n = side * side
    else:
        a = gra.generate_random_regular(n // 2, 4, seed=3)
        adj = sp.block_diag([a, a]).tocsr()                # two components: a 2-dimensional null space
    want = D + 1
    emb, info = laplacian_embedding_hip(adj, D, return_info=True, tol=1e-10)
    assert emb.shape == (n, D) and emb.dtype == np.float32 and np.isfinite(emb).all()
    assert info["converged"]
    L, vals, vecs = _reference_eig(adj, want + 4)
    np.testing.assert_allclose(info["eigenvalues"], vals[:want], atol=1e-8)
    X = info["vectors_all"]
    assert np.abs(X.T @ X - np.eye(want)).max() < 1e-8     # orthonormal Ritz vectors
    assert np.abs(L @ X - X * info["eigenvalues"]).max() < 1e-7
    # subspace agreement wherever the wanted set ends at a spectral gap
    if vals[want] - vals[want - 1] > 1e-6:
        P = vecs[:, :want]
        assert np.linalg.norm(X - P @ (P.T @ X)) < 1e-6


def test_embedder_init_option_and_layout_runs():
    import graphem_rapids_amd as gra
    adj = gra.generate_random_regular(2000, 6, seed=5)
    emb = gra.create_graphem(adj, n_components=3, backend="hip", verbose=False, seed=0, init="laplacian_hip")
    p0 = emb.get_positions()
    assert p0.shape == (2000, 3)
    # same subspace as the reference's own start (scipy eigsh, pt.py:364-365)
    ref = gra.create_graphem(adj, n_components=3, backend="hip", verbose=False, seed=0, init="laplacian").get_positions()
    q, _ = np.linalg.qr(ref.astype(np.float64))
    assert np.linalg.norm(p0 - q @ (q.T @ p0)) < 1e-4
    out = emb.run_layout(5)
    assert np.isfinite(out).all()


def test_spans_the_reference_held_start_of_c1():
    """on BASELINE configs[0]'s graph the GPU solver must span what the REFERENCE itself started
    from -- `p0` of tests/golden/c1_er1000.npz is the reference's own Laplacian embedding (pt.py:364-365, ARPACK).
    C1 has isolated vertices and small components, so eigenvalue 0 is degenerate and the embedding is any basis of a
    part of that null space: compare as subspaces of the wanted eigenspace, and check every reference column is an
    eigenvector combination the solver's operator accepts (residual)."""
    import graphem_rapids_amd as gra
    from conftest import load_golden
    from graphem_rapids_amd.spectral import laplacian_embedding_hip
    g = load_golden("c1_er1000")
    n, D = int(g["n"]), int(g["D"])
    adj = gra.edges_to_adjacency(n, g["edges"])
    L, vals, vecs = _reference_eig(adj, n)
    p0 = g["p0"].astype(np.float64)
    # the reference's columns are (to fp32) eigenvectors of the same Laplacian, each for one eigenvalue lam_j
    lam = np.array([(p0[:, j] @ (L @ p0[:, j])) / (p0[:, j] @ p0[:, j]) for j in range(D)])
    for j in range(D):
        r = L @ p0[:, j] - lam[j] * p0[:, j]
        assert np.linalg.norm(r) <= 1e-4 * np.linalg.norm(p0[:, j])
    emb, info = laplacian_embedding_hip(adj, D, return_info=True, tol=1e-10)
    assert info["converged"]
    # wanted eigenvalues: the D+1 smallest; the solver's must equal the dense ones, and the reference's Rayleigh
    # quotients must lie among them
    np.testing.assert_allclose(np.sort(info["eigenvalues"][: D + 1]), vals[: D + 1], atol=1e-7)
    top = vals[D]
    assert np.all(lam <= top + 1e-5)
    # both embeddings lie in the eigenspace of eigenvalues <= top (its dimension exceeds D + 1 when 0 is degenerate)
    basis = vecs[:, vals <= top + 1e-7]
    for M in (p0, emb.astype(np.float64)):
        Q, _ = np.linalg.qr(M)
        resid = Q - basis @ (basis.T @ Q)
        assert np.abs(resid).max() <= 2e-4
    if vals[1] - vals[0] > 1e-6 and vals[D + 1] - vals[D] > 1e-6:   # connected, and a gap behind the wanted set: THE subspace
        Qa, _ = np.linalg.qr(p0)
        Qb, _ = np.linalg.qr(emb.astype(np.float64))
        sv = np.linalg.svd(Qa.T @ Qb, compute_uv=False)
        assert sv.min() >= 1.0 - 1e-6, sv


@pytest.mark.gpu
def test_spans_the_references_own_eigsh_start_at_100k():
    """BASELINE configs[1]'s graph (the reference's generate_random_regular(100000, 8, seed=0)) and the
    start the REFERENCE computed for it with scipy eigsh (pt.py:337-379; tests/golden/make_golden_spectral.py, 18 s
    there).  The GPU solver must return the same three eigenpairs: eigenvalues equal to the reference columns' Rayleigh
    quotients (0.338738, 0.339143, 0.339354: gaps of 2-4e-4 at the edge of a random regular graph's spectrum), and the
    same subspace -- in under a second... of solver time (reported)."""
    import time
    import graphem_rapids_amd as gra
    from graphem_rapids_amd.spectral import laplacian_embedding_hip
    import hashlib
    import os
    from conftest import GOLDEN_DIR
    g = np.load(os.path.join(GOLDEN_DIR, "spectral_rr100k.npz"))
    n, D = int(g["n"]), int(g["D"])
    p0 = g["p0"].astype(np.float64)
    # the fixture's graph: rebuilt here from the reference-held edge list of c2_rr100k.npz (the same generator call)
    edges = np.ascontiguousarray(np.load(os.path.join(GOLDEN_DIR, "c2_rr100k.npz"))["edges"], dtype=np.int32)
    assert hashlib.sha1(edges.tobytes()).hexdigest() == str(g["edges_sha1"])
    adj = gra.edges_to_adjacency(n, edges)
    t0 = time.perf_counter()
    emb, info = laplacian_embedding_hip(adj, D, return_info=True, tol=1e-9)
    took = time.perf_counter() - t0
    assert info["converged"]
    lam = np.sort(np.asarray(info["eigenvalues"])[1: D + 1])
    np.testing.assert_allclose(lam, g["rayleigh"], atol=2e-7)
    Qa, _ = np.linalg.qr(p0)
    Qb, _ = np.linalg.qr(emb.astype(np.float64))
    sv = np.linalg.svd(Qa.T @ Qb, compute_uv=False)
    print(f"\nlaplacian_hip at n = 100 K: {took:.2f} s, {info.get('matvecs')} matvecs; smallest singular value of Qa^T Qb = {sv.min():.8f}")
    assert sv.min() >= 1.0 - 1e-5, sv


@pytest.mark.gpu
def test_sweep_kernels_equal_the_torch_steps():
    """gh_trlan_sweep (csrc/spectral.hip: matvec + classical Gram-Schmidt twice as kernels) against the same solver with
    torch GEMVs: same eigenvalues on a graph with isolated vertices and a degenerate spectrum (all five wanted eigenvalues
    are 0 there, whatever the solver does) and on a connected one, where they are not.  Every returned column x_j of
    either method is an eigenvector to its eigenvalue: |L x_j - lambda_j x_j| <= 4 tol |x_j| -- tol bounds the Ritz
    estimate |B y - theta y| / theta, theta <= 2 on B, and 2 for the gap between the estimate and the true residual."""
    import graphem_rapids_amd as gra
    from graphem_rapids_amd.spectral import laplacian_embedding_hip
    n, tol = 30000, 1e-9
    graphs = {"er": gra.edges_to_adjacency(n, gra.erdos_renyi_edges(n, 4.0 / n, seed=5)),   # mean degree 4: isolated
              "rr": gra.generate_random_regular(n, 6, seed=5)}                              # vertices, small components
    for name, adj in graphs.items():
        sym = sp.csr_matrix(adj + adj.transpose())
        sym.data = np.ones_like(sym.data)
        L = laplacian(sym, normed=True)                   # as _reference_eig, but sparse
        out = {}
        for method in ("trlan", "trlan_torch"):
            emb, info = laplacian_embedding_hip(adj, 4, return_info=True, tol=tol, method=method)
            assert info["converged"]
            lam, X = np.asarray(info["eigenvalues"])[:5], info["vectors_all"]
            assert emb.shape == (n, 4) and X.shape == (n, 5)
            resid = np.linalg.norm(L @ X - X * lam, axis=0) / np.linalg.norm(X, axis=0)
            print(f"\n{name} {method}: eigenvalues {lam}, residuals {resid}")
            assert np.all(resid <= 4 * tol), (name, method, resid)
            out[method] = np.sort(lam)
        np.testing.assert_allclose(out["trlan"], out["trlan_torch"], atol=1e-8)
        if name == "rr":                                  # connected: one zero eigenvalue, then the spectral gap
            for lam in out.values():
                assert lam[0] < 1e-8 < lam[1]
