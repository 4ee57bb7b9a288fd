"""The float64 engine (csrc/f64.hip, gh_create_f64; dtype=torch.float64 on the public class) against fixtures the REFERENCE
produced computing in float64 (tests/golden/make_golden.py cases *_f64: create_graphem(..., dtype=torch.float64), pt.py:56;
the reference's own test of this is tests/test_pytorch_backend.py:169-181).  Needs a real MI355X."""
import os

import numpy as np
import pytest

import f64_reference as reference
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", ["c1_er1000_f64", "d16_er2000_f64"])
def test_every_phase_and_one_step_in_float64(case):
    from graphem_rapids_amd import _native
    g = np.load(os.path.join(GOLDEN_DIR, case + ".npz"))
    n, D, k, S = int(g["n"]), int(g["D"]), int(g["k"]), int(g["S"])
    Lm, ka, ki = (float(x) for x in g["params"])
    eng = _native.Engine(n, D, g["edges"], Lm, ka, ki, k, S, dtype="float64")
    worst = {}
    for t in g["steps"]:
        pos, sampled = g[f"pos_{t}"], g[f"sampled_{t}"]
        assert pos.dtype == np.float64
        eng.set_positions(pos)
        assert np.array_equal(eng.get_positions(), pos)
        F = eng.spring_forces()
        ref = g[f"F_spring_{t}"]
        worst["spring"] = max(worst.get("spring", 0.0), float(np.abs(F - ref).max() / max(1.0, np.abs(ref).max())))
        knn = eng.knn_midpoints(sampled)
        assert np.array_equal(knn, g[f"knn_{t}"]), f"{case} step {t}: neighbour ids"
        Fi = eng.intersection_forces(sampled, g[f"knn_{t}"])
        ref = g[f"F_inter_{t}"]
        worst["inter"] = max(worst.get("inter", 0.0), float(np.abs(Fi - ref).max() / max(1.0, np.abs(ref).max())))
        eng.step(sampled)
        out = eng.get_positions()
        assert out.dtype == np.float64
        worst["p2"] = max(worst.get("p2", 0.0), float(np.abs(out - g[f"pos_next_{t}"]).max()))
    eng.close()
    print(f"\n{case}: float64 engine vs the reference in float64:", worst)
    assert worst["spring"] <= 1e-13 and worst["inter"] <= 1e-12 and worst["p2"] <= 1e-10, worst


def test_float64_trajectory_and_public_api():
    """Three iterations with the reference's sample stream stay within 1e-9 of its float64 trajectory; the public class
    with dtype=torch.float64 computes in float64 (tests/test_pytorch_backend.py:169-181 checks dtype plumbing only)."""
    import torch
    import graphem_rapids_amd as gra
    from graphem_rapids_amd import _native
    g = np.load(os.path.join(GOLDEN_DIR, "c1_er1000_f64.npz"))
    n, D, k, S = int(g["n"]), int(g["D"]), int(g["k"]), int(g["S"])
    eng = _native.Engine(n, D, g["edges"], 1.0, 0.2, 0.5, k, S, dtype="float64")
    eng.set_positions(g["p0"])
    eng.run(3, g["sample_stream"][:3])
    assert np.abs(eng.get_positions() - g["pos_next_2"]).max() <= 1e-9
    eng.run(2)            # device sampler
    assert np.isfinite(eng.get_positions()).all()
    eng.close()
    adj = gra.edges_to_adjacency(n, g["edges"])
    emb = gra.create_graphem(adj, n_components=3, backend="hip", verbose=False, seed=0, dtype=torch.float64, sampler="torch")
    assert emb.dtype == torch.float64 and emb._positions.dtype == torch.float64 and emb.positions.dtype == np.float64
    # the spectral start reaches the float64 engine unrounded (pt.py:372-376 casts the float64 eigenvectors to dtype): it
    # carries more than float32 precision and is the reference's own float64 start up to the sign of an eigenvector and
    # ARPACK's run-to-run noise
    start = emb.positions
    assert np.abs(start - start.astype(np.float32).astype(np.float64)).max() > 0
    for d in range(D):
        assert min(np.abs(start[:, d] - g["p0"][:, d]).max(), np.abs(start[:, d] + g["p0"][:, d]).max()) <= 1e-6
    emb.positions = g["pos_0"]
    torch.manual_seed(7)
    ids = torch.randperm(len(g["edges"]))[:S].numpy()
    torch.manual_seed(7)
    emb.update_positions()
    eng = _native.Engine(n, D, g["edges"], 1.0, 0.2, 0.5, k, S, dtype="float64")
    eng.set_positions(g["pos_0"])
    eng.step(ids.astype(np.int32))
    np.testing.assert_allclose(emb.positions, eng.get_positions(), rtol=0, atol=1e-12)   # (double atomics: the order of the handful of terms a vertex receives varies)
    out = emb.run_layout(4)
    assert out.dtype == np.float64 and np.isfinite(out).all()
    np.testing.assert_allclose(out.std(0, ddof=1), 1.0, atol=1e-5)
    with pytest.raises(ValueError):
        eng.lib  # noqa: B018
        _native.Engine(n, D, g["edges"], 1.0, 0.2, 0.5, k, S, dtype="float64", partition=(0, n // 2, 0, 0, 1))
    eng.close()


@pytest.mark.gpu
def test_float64_search_against_numpy_with_one_stripe_holding_the_best():
    """The float64 search keeps the four smallest keys of a thread's stripe (ids = threadIdx.x mod 256) from one scan and
    rescans the stripe when more of the K best sit in it (csrc/f64.hip f64_knn_kernel).  A perfect matching makes every
    midpoint free to place: here the 16 midpoints nearest the query all have ids = 7 mod 256 -- one thread hands over every
    neighbour -- and a second query sees random midpoints; both rows against a float64 brute force in numpy (ties on the
    smaller id; column 0 dropped, pt.py:421)."""
    from graphem_rapids_amd import _native
    rng = np.random.default_rng(5)
    E, D, k = 4096, 3, 12
    n = 2 * E
    edges = np.stack([np.arange(0, n, 2), np.arange(1, n, 2)], axis=1).astype(np.int32)
    mid = rng.standard_normal((E, D)) * 3.0 + 10.0
    mid[0] = 0.0                                            # query A at the origin
    for j in range(16):
        mid[7 + 256 * j] = np.array([0.01 * (j + 1), 0.0, 0.0])
    mid[100] = mid[200]                                     # a tie for query B's list to order by id
    pos = np.repeat(mid, 2, axis=0)                         # both endpoints on the midpoint
    eng = _native.Engine(n, D, edges, 1.0, 0.2, 0.5, k, 2, dtype="float64")
    eng.set_positions(pos)
    sampled = np.array([0, 150], dtype=np.int32)
    knn = eng.knn_midpoints(sampled)
    for row, q in zip(knn, sampled):
        d2 = ((mid - mid[q]) ** 2).sum(axis=1)              # (fma chain vs numpy's sum: equal here up to the last bit; the
        order = np.lexsort((np.arange(E), d2))              #  rows below are separated by far more)
        assert np.array_equal(row, order[1:k + 1]), (q, row, order[1:k + 1])
    assert list(knn[0]) == [7 + 256 * j for j in range(12)]
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("D,k,S,kind", [(3, 10, 64, "gauss"), (2, 5, 32, "gauss"), (5, 16, 48, "gauss"), (16, 32, 16, "gauss"),
                                        (7, 10, 16, "gauss"), (3, 10, 32, "collapsed"), (3, 10, 24, "clones"), (4, 10, 32, "gauss"),
                                        (1, 5, 16, "gauss"), (2, 10, 32, "collapsed"), (3, 10, 16, "far"), (6, 10, 32, "gauss"),
                                        (8, 10, 32, "gauss")])
def test_float64_filtered_search_equals_a_numpy_brute_force(D, k, S, kind):
    """From 131072 edges on the float64 engine searches through a filter (csrc/f64.hip: per query an exclusive bound from
    every stride-th midpoint, one reference-major pass over all midpoints that parks what lies below it, the exact
    (double distance, id) ranking over the parked ones).  Rows against a float64 brute force in numpy over all midpoints
    (ties on the smaller id, column 0 dropped, pt.py:421) -- on a Gaussian cloud, on a cloud collapsed to 1e-9 around a
    far point (float keys of many distances coincide), and with every position shared by 64 vertices (ties in every
    row; parked lists overflow and the query falls back to the full passes), and on a cloud outside the f16 range of the
    matrix-pipe pre-filter (two and three components: such midpoints are scanned in double, such queries take the full passes).
    Every instantiation of the filter runs: matrix pipe (D = 2, 3), F64_FILTER(4, 4), (5, 2), (6, 2), (8, 2), (16, 2) and the
    run-time one (D = 1, 7).  Then one step on those rows against tests/f64_reference.py."""
    import graphem_rapids_amd as gra
    from graphem_rapids_amd import _native
    rng = np.random.default_rng(D * 100 + k)
    n = 40000
    edges = np.ascontiguousarray(gra.random_regular_edges(n, 8, seed=D), dtype=np.int32)
    E = len(edges)
    assert E >= 131072
    if kind == "gauss":
        pos = rng.standard_normal((n, D))
    elif kind == "collapsed":
        pos = rng.standard_normal((n, D)) * 1e-9 + 5.0
    elif kind == "far":      # a cloud beyond the f16 range of the matrix-pipe pre-filter (|coordinate| > 128) plus a few near points
        pos = rng.standard_normal((n, D)) * 40.0 + 300.0
        pos[: n // 20] = rng.standard_normal((n // 20, D))
    else:
        pos = np.repeat(rng.standard_normal((n // 64, D)), 64, axis=0)
    eng = _native.Engine(n, D, edges, 1.0, 0.2, 0.5, k, S, dtype="float64")
    eng.set_positions(pos)
    sampled = rng.permutation(E)[:S].astype(np.int32)
    knn = eng.knn_midpoints(sampled)
    mid = (pos[edges[:, 0]] + pos[edges[:, 1]]) / 2.0
    bad = 0
    for row, q in zip(knn, sampled):
        diff = mid[q][None, :] - mid
        d2 = np.zeros(E)
        for d in range(D):          # the engine's chain: fma(diff_d, diff_d, acc) in coordinate order; numpy rounds the
            d2 = d2 + diff[:, d] * diff[:, d]   # product separately -- rows may differ where two distances agree to the last bits
        order = np.lexsort((np.arange(E), d2))[1:k + 1]
        if not np.array_equal(row, order):
            # accept a difference only between midpoints whose distances agree to 4 ulps (fma vs separate rounding)
            a, b = np.sort(d2[row]), np.sort(d2[order])
            assert np.allclose(a, b, rtol=1e-15, atol=0), (q, row, order)
            bad += 1
    assert bad <= (S if kind != "gauss" else 1)
    # ... and the step runs on it (there is no switch onto the full passes: the small-graph tests above cover those): with
    # the rows just checked, one step equals the extended-precision iteration of tests/f64_reference.py on exactly those
    # rows, within the one-step bar of test_every_phase_and_one_step_in_float64.  (The two collapsed clouds measured 1.9e-5
    # while f64_intersect_kernel subtracted the rounded centre (p1 + p2 + q1 + q2) / 4 from an endpoint 1e-9 away from it;
    # 1.9e-14 since it averages the four differences.)
    eng.step(sampled)
    out = eng.get_positions()
    eng.close()
    assert np.isfinite(out).all()
    err = float(np.abs(out - reference.step(pos, edges, sampled, knn, 1.0, 0.2, 0.5)).max())
    print(f"\nfiltered step D={D} k={k} S={S} {kind}: {err:.3e} of bar 1e-10")
    assert err <= 1e-10
