"""gh_gen_* (csrc/generators.hip) on the device: against the restatement of the header's rules (tests/generators_reference.py)
bit for bit, against the library's host path at sizes the restatement cannot reach, against itself (runs, memory budgets),
at its limits, and through the three benchmark entry points with the reference's example parameters."""
import numpy as np
import pytest

import graphem_rapids_amd as gr
from graphem_rapids_amd import _native
import generators_reference as ref
import launch_caps as lc
from test_generators_cpu import BA_GRID, GEOMETRIC_GRID, SBM_GRID

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device():
    g = _native.Generator(0)
    yield g
    g.close()


@pytest.fixture(scope="module")
def host():
    g = _native.Generator(-1)
    yield g
    g.close()


@pytest.mark.parametrize("sizes,P,seed", SBM_GRID)
def test_sbm_device_equals_restatement(device, sizes, P, seed):
    assert np.array_equal(device.sbm(sizes, P, seed), ref.sbm_edges(sizes, P, seed))


@pytest.mark.parametrize("n,radius,dim,seed", GEOMETRIC_GRID)
def test_geometric_device_equals_restatement(device, n, radius, dim, seed):
    edges, pos = device.geometric(n, radius, dim, seed)
    want, want_pos = ref.geometric_edges(n, radius, dim, seed)
    assert np.array_equal(edges, want)
    assert np.array_equal(pos, want_pos)


@pytest.mark.parametrize("n,m,seed", BA_GRID)
def test_ba_device_equals_restatement(device, n, m, seed):
    assert np.array_equal(device.ba(n, m, seed), ref.ba_edges(n, m, seed))


def big_sbm():
    """200 K vertices in 50 unequal blocks, about 3 M edges."""
    sizes = 2000 + 80 * np.arange(50)          # 2000 .. 5920, sum 198 000 ... plus the remainder in the last block
    sizes[-1] += 200_000 - sizes.sum()
    rng = np.random.default_rng(5)
    P = rng.uniform(2e-5, 8e-5, size=(50, 50))
    P = (P + P.T) / 2
    np.fill_diagonal(P, rng.uniform(2e-3, 8e-3, size=50))
    P[3, 7] = P[7, 3] = 0.0
    return sizes, P


def test_sbm_device_equals_host_200k(device, host):
    sizes, P = big_sbm()
    d = device.sbm(sizes, P, 11)
    h = host.sbm(sizes, P, 11)
    print(f"sbm 200 K vertices, 50 blocks: {len(d)} edges")
    assert len(d) > 1_000_000
    assert np.array_equal(d, h)


def test_sbm_device_equals_host_past_the_cap(device, host):
    """Two blocks of 550 000 vertices, empty inside and joined by p = 1e-6: 36.9 M segments against the 65 536 * 256 that
    gen_sbm_kernel takes a trip, the live block pair across the end of the first (tests/launch_caps.py, SBM)."""
    sizes, p = list(lc.SBM["sizes"]), lc.SBM["p"]
    P = [[0.0, p], [p, 0.0]]
    d = device.sbm(sizes, P, 11)
    h = host.sbm(sizes, P, 11)
    assert 290_000 < len(d) < 315_000   # p * 550 000^2 = 302 500, standard deviation 550
    assert (d[:, 0] < sizes[0]).all() and (d[:, 1] >= sizes[0]).all()
    assert np.array_equal(d, h)


@pytest.mark.parametrize("dim,radius", [(2, 0.002523), (3, 0.01684)])
def test_geometric_device_equals_host_500k(device, host, dim, radius):
    n = 500_000
    d, dp = device.geometric(n, radius, dim, 21)
    h, hp = host.geometric(n, radius, dim, 21)
    print(f"geometric n = {n}, dim = {dim}: mean degree {2 * len(d) / n:.2f}")
    assert 8 < 2 * len(d) / n < 12
    assert np.array_equal(d, h)
    assert np.array_equal(dp, hp)


def test_ba_device_equals_host_1m(device, host):
    n, m = 1_000_000, 4
    d = device.ba(n, m, 31)
    print(f"ba n = {n}, m = {m}: {device.rounds} rounds")
    assert len(d) == m * (n - m)
    assert 1 <= device.rounds <= 4096
    assert np.array_equal(d, host.ba(n, m, 31))


def test_invariance_across_runs_and_budgets():
    sizes, P = [3000, 5000, 2000], np.array([[0.01, 0.001, 0.002], [0.001, 0.02, 0.0], [0.002, 0.0, 1.0]])
    results = []
    for budget in (0, 0, 96 << 20, 16 << 30):
        g = _native.Generator(0)
        g.set_memory_budget(budget)
        e, p = g.geometric(60_000, 0.01, 3, 4)
        results.append((g.sbm(sizes, P, 2), e, p, g.ba(50_000, 5, 3)))
        g.close()
    for other in results[1:]:
        for a, b in zip(results[0], other):
            assert np.array_equal(a, b)


def test_over_budget_is_an_error_before_anything_is_written():
    g = _native.Generator(0)
    # a radius that makes the graph complete: n (n - 1) / 2 = 5 * 10^9 edges, 80 GB of keys
    with pytest.raises(MemoryError, match=r"4999950000 edges need \d+ bytes, the memory budget is \d+"):
        g.geometric(100_000, 2.0, 2, 0)
    with pytest.raises(MemoryError, match="memory budget"):
        g.sbm([60_000, 60_000], [[1.0, 1.0], [1.0, 1.0]], 0)
    g.set_memory_budget(1 << 20)
    with pytest.raises(MemoryError, match="memory budget"):
        g.ba(100_000, 4, 0)
    # the handle still works, and a result that fits is whole
    g.set_memory_budget(0)
    edges, _ = g.geometric(2000, 2.0, 2, 0)
    assert len(edges) == 2000 * 1999 // 2
    g.close()


def test_public_functions_take_the_device_past_the_crossover(device):
    n = 2 * gr.generators.DEVICE_MIN_VERTICES
    edges, rounds = gr.barabasi_albert_edges(n, 3, seed=9, return_rounds=True)
    assert rounds >= 1                                       # the device ran (the host path reports 0)
    assert edges.dtype == np.int64 and np.array_equal(edges, device.ba(n, 3, 9))
    small, rounds = gr.barabasi_albert_edges(300, 3, seed=9, return_rounds=True)
    assert rounds == 0 and np.array_equal(small, device.ba(300, 3, 9))


def test_benchmarks_run_on_the_new_generators():
    res = gr.run_benchmark(gr.generate_sbm, {"n_per_block": 125, "num_blocks": 4, "p_in": 0.3, "p_out": 0.01, "seed": 42})
    for key in ("n", "m", "density", "avg_degree", "layout_time", "graph_type", "n_components", "backend", "radii", "positions",
                "degree", "betweenness", "eigenvector", "pagerank", "closeness", "node_load", "total_time"):
        assert key in res, key
    assert res["n"] == 500 and res["graph_type"] == "generate_sbm"
    res = gr.benchmark_correlations(gr.generate_ba, {"n": 500, "m": 2, "seed": 42})
    assert res["m"] == 2 * 498
    assert set(res["correlations"]) == {"degree", "betweenness", "eigenvector", "pagerank", "closeness", "node_load"}
    res = gr.run_influence_benchmark(gr.generate_ws, {"n": 100, "k": 4, "p": 0.1, "seed": 42})
    for key in ("graph_type", "n", "m", "graphem_seeds", "greedy_seeds", "graphem_influence", "greedy_influence",
                "random_influence", "graphem_time", "greedy_time", "graphem_norm_influence", "greedy_norm_influence",
                "random_norm_influence", "graphem_efficiency", "greedy_efficiency", "total_time"):
        assert key in res, key
    assert res["n"] == 100 and res["m"] == 200
