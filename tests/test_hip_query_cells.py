"""The query-cell pre-filter of the fused spring+scan kernel (csrc/qcell_core.h, spring_scan_cells_kernel) against the
split-f16 MFMA pre-filter on the same engine state: both keep exactly the pairs with fp32 d2 <= tau, so the neighbour
rows must be identical and a run must give the same positions bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, DEG, K = 50000, 8, 10          # 200 000 edges: 391 fused workgroups
S_MAX = 256                       # largest sample size the query-cell filter takes (GH_QC_SMAX)


def _graph():
    import graphem_rapids_amd as gra
    return gra.random_regular_edges(N, DEG, seed=21).astype(np.int32)


def _engine(D, S, dist="exact", edges=None, n=N, seed=3):
    from graphem_rapids_amd import _native
    edges = _graph() if edges is None else edges
    return _native.Engine(n, D, edges, 1.0, 0.2, 0.5, K, S, seed=seed, knn_distance=dist)


def _state(kind, D, edges, rng):
    pos = (rng.standard_normal((N, D)) * 0.1).astype(np.float32)   # the reference's random start
    if kind == "random":
        return pos
    if kind == "iter200":
        eng = _engine(D, 256, edges=edges)
        eng.set_positions(pos)
        eng.run(200)
        out = eng.get_positions()
        eng.close()
        return out
    if kind == "outliers":   # a few vertices 1e5 sigma out: the end cells run to +-inf
        far = rng.permutation(N)[:50]
        pos[far] *= np.float32(1e5) * np.sign(rng.standard_normal((50, 1))).astype(np.float32)
        return pos
    if kind == "collapsed":   # duplicated positions, and a third of the graph collapsed onto one point
        pos[1::2] = pos[0::2]
        pos[: N // 3] = pos[7]
        return pos
    if kind == "lattice":     # integer lattice: coordinates -- and so the quantile boundaries -- sit on each other
        return rng.integers(-2, 3, size=(N, D)).astype(np.float32)
    if kind == "nonfinite":   # vertices at +inf: their midpoints' queries get non-finite coordinates and tau
        pos[rng.permutation(N)[:3], 0] = np.inf
        return pos
    raise ValueError(kind)


def _sample(kind, S, edges, pos, rng):
    sampled = rng.permutation(len(edges))[:S].astype(np.int32)
    if kind == "nonfinite" and S > 1:
        bad = np.nonzero(~np.isfinite(pos[edges].sum(axis=(1, 2))))[0]
        sampled[: min(len(bad), S // 2)] = bad[: S // 2]
    if kind == "outliers" and S > 1:
        far = np.nonzero(np.abs(pos[edges]).max(axis=(1, 2)) > 1e3)[0]
        sampled[: min(len(far), S // 4)] = far[: S // 4]
    return sampled


STATES = ["random", "iter200", "outliers", "collapsed", "lattice", "nonfinite"]


@pytest.fixture(scope="module")
def edges():
    return _graph()


@pytest.mark.parametrize("kind", STATES)
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("dist", ["exact", "cdist"])
def test_cells_and_mfma_give_the_same_rows(kind, D, dist, edges):
    rng = np.random.default_rng(10 * STATES.index(kind) + D)
    pos = _state(kind, D, edges, rng)
    for S in (1, 33, S_MAX):
        sampled = _sample(kind, S, edges, pos, rng)
        eng = _engine(D, S, dist, edges=edges)
        eng.set_positions(pos)
        rows = {}
        for mode in ("mfma", "cells", "mfma"):   # and back: the engine switches the threshold placement both ways
            eng.set_scan_filter(mode)
            assert eng.scan_filter() == mode
            got = eng.knn_midpoints(sampled)
            if mode in rows:
                assert np.array_equal(rows[mode], got), (kind, D, dist, S, "mfma twice")
            rows[mode] = got
        eng.close()
        assert np.array_equal(rows["mfma"], rows["cells"]), (kind, D, dist, S)


@pytest.mark.parametrize("D,S", [(2, 256), (3, 256), (3, 33)])
def test_fifty_iterations_give_the_same_positions(D, S, edges):
    pos = (np.random.default_rng(D).standard_normal((N, D)) * 0.1).astype(np.float32)
    out = {}
    for mode in ("mfma", "cells"):
        eng = _engine(D, S, edges=edges, seed=11)
        eng.set_scan_filter(mode)
        eng.set_positions(pos)
        eng.run(50)
        out[mode] = eng.get_positions()
        eng.close()
    assert out["mfma"].tobytes() == out["cells"].tobytes()


def test_auto_rule_and_refusals(edges):
    import graphem_rapids_amd as gra
    eng = _engine(3, 256, edges=edges)   # 391 workgroups: thresholds inside the fused launch, so the MFMA filter
    assert eng.scan_filter() == "mfma"
    eng.close()
    big = gra.random_regular_edges(300000, 8, seed=2).astype(np.int32)   # 2344 workgroups: a threshold launch of its own
    eng = _engine(3, 256, edges=big, n=300000)
    assert eng.scan_filter() == "cells"
    eng.close()
    eng = _engine(3, S_MAX + 1, edges=big, n=300000)
    assert eng.scan_filter() == "mfma"
    with pytest.raises(Exception):
        eng.set_scan_filter("cells")
    eng.close()
    eng = _engine(4, 256, edges=edges)
    assert eng.scan_filter() == "auto"   # D = 4: the wide form, neither filter
    with pytest.raises(Exception):
        eng.set_scan_filter("cells")
    eng.close()


def test_large_graph_cells_match_mfma_over_a_run():
    """A graph whose AUTO choice is the cell table (thresholds in a launch of their own), both filters over a run."""
    import graphem_rapids_amd as gra
    n = 300000
    big = gra.random_regular_edges(n, 8, seed=4).astype(np.int32)
    pos = (np.random.default_rng(9).standard_normal((n, 3)) * 0.1).astype(np.float32)
    out = {}
    for mode in ("cells", "mfma"):
        eng = _engine(3, 256, edges=big, n=n, seed=5)
        eng.set_scan_filter(mode)
        eng.set_positions(pos)
        eng.run(30)
        out[mode] = eng.get_positions()
        eng.close()
    assert out["mfma"].tobytes() == out["cells"].tobytes()
