"""Centrality layer without a GPU: the exported C ABI, the reference's benchmark signatures, networkx's choice of sampled
sources, host-side argument checks, and the numpy restatement (tests/centrality_reference.py) against networkx."""
import ctypes
import inspect
import os
import random

import networkx as nx
import numpy as np
import pytest

import graphem_rapids_amd as gr
from graphem_rapids_amd import _native
from graphem_rapids_amd import centrality as cent

import centrality_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CENT_SYMBOLS = ["gh_cent_create", "gh_cent_destroy", "gh_cent_last_error", "gh_cent_edge_count", "gh_cent_csr_device",
                "gh_cent_set_memory_budget", "gh_cent_paths", "gh_cent_pagerank", "gh_spmv_adj_shift"]

REFERENCE_PARAMS = ["graph_generator", "graph_params", "dim", "L_min", "k_attr", "k_inter", "n_neighbors", "sample_size",
                    "num_iterations", "backend"]


def _lib():
    from graphem_rapids_amd import build as gra_build
    gra_build.build()
    return _native.load()


def test_centrality_symbols_declared_exported_and_listed():
    header = open(os.path.join(ROOT, "include", "graphem_hip.h")).read()
    _lib()
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in CENT_SYMBOLS:
        assert name + "(" in header, name
        assert name in _native.SYMBOLS, name
        assert hasattr(lib, name), name


@pytest.mark.parametrize("fn", ["run_benchmark", "benchmark_correlations"])
def test_benchmark_functions_have_the_reference_parameters(fn):
    f = getattr(gr, fn)
    params = inspect.signature(f).parameters
    assert list(params)[:len(REFERENCE_PARAMS)] == REFERENCE_PARAMS
    assert params["dim"].default == (3 if fn == "run_benchmark" else 2)
    assert params["L_min"].default == 10.0 and params["num_iterations"].default == 40
    assert params["betweenness_k"].kind == inspect.Parameter.KEYWORD_ONLY
    assert any(p.kind == inspect.Parameter.VAR_KEYWORD for p in params.values())


@pytest.mark.parametrize("n,k,seed", [(50, 10, 0), (300, 100, 7), (1000, 64, 123), (20, 20, 3)])
def test_sampled_sources_are_networkx_choice(n, k, seed):
    G = nx.gnp_random_graph(n, 0.05, seed=seed)
    assert cent.sample_sources(G.nodes(), k, seed) == random.Random(seed).sample(list(G.nodes()), k)
    # and what networkx's seeded betweenness actually sums over: restate it over our sample
    if n <= 300:
        src = cent.sample_sources(G.nodes(), k, seed)
        bc, _, _, _ = ref.paths(n, np.array(G.edges()).reshape(-1, 2), src)
        want = nx.betweenness_centrality(G, k=k, seed=seed)
        got = bc * cent.betweenness_scale(n, True, k)
        np.testing.assert_allclose(got, [want[i] for i in range(n)], rtol=1e-9, atol=1e-12)


def test_sampled_sources_with_labels():
    G = nx.relabel_nodes(nx.path_graph(40), {i: f"v{i}" for i in range(40)})
    assert cent.sample_sources(G.nodes(), 5, 11) == random.Random(11).sample(list(G.nodes()), 5)


def _no_device_graph(n=10):
    """A CentralityGraph whose device handle is a stub that fails the test if touched."""
    class Boom:
        def __getattr__(self, name):
            raise AssertionError(f"device call {name} reached")
    g = cent.CentralityGraph.__new__(cent.CentralityGraph)
    g.n, g.edges, g.labels, g.device_id = n, np.zeros((0, 2), dtype=np.int64), None, 0
    g._g = Boom()
    return g


def test_host_validation_before_any_device_call():
    g = _no_device_graph()
    with pytest.raises(ValueError):
        g.pagerank(alpha=1.5)
    with pytest.raises(ValueError):
        g.pagerank(alpha=-0.1)
    with pytest.raises(ValueError):
        g.pagerank(max_iter=0)
    with pytest.raises(ValueError):
        g.set_memory_budget(-1)
    with pytest.raises(ValueError):
        g.raw_paths([0, 10])
    with pytest.raises(ValueError):
        g.raw_paths([-1])
    with pytest.raises(ValueError):
        g.betweenness(k=11)
    with pytest.raises(ValueError):
        g.eigenvector(shift=0.0)
    with pytest.raises(ValueError):   # _graph_arcs: an endpoint outside [0, n)
        cent.CentralityGraph(np.array([[0, 5]]), n=3)
    with pytest.raises(NotImplementedError):
        cent.CentralityGraph(nx.DiGraph([(0, 1)]))
    with pytest.raises(NotImplementedError):
        gr.betweenness_centrality(nx.path_graph(4), endpoints=True)
    with pytest.raises(NotImplementedError):
        gr.betweenness_centrality(nx.path_graph(4), weight="weight")
    with pytest.raises(NotImplementedError):
        gr.load_centrality(nx.path_graph(4), cutoff=2)
    with pytest.raises(NotImplementedError):
        gr.closeness_centrality(nx.path_graph(4), distance="weight")
    with pytest.raises(NotImplementedError):
        gr.pagerank(nx.path_graph(4), personalization={0: 1})
    G = nx.path_graph(4)
    G.add_edge(0, 1, weight=2.0)
    with pytest.raises(NotImplementedError):
        gr.pagerank(G)


def test_c_abi_rejects_bad_arguments_without_a_device():
    lib = _lib()
    h = ctypes.c_void_p()
    bad = np.array([[0, 1], [2, 7]], dtype=np.int32)
    assert lib.gh_cent_create(ctypes.byref(h), 0, 5, 2, _native.ptr(bad)) == _native.GH_ERR_INVALID
    assert not h.value
    assert b"outside" in lib.gh_cent_last_error(None)
    assert lib.gh_cent_create(ctypes.byref(h), 0, 0, 0, None) == _native.GH_ERR_INVALID
    assert lib.gh_cent_set_memory_budget(None, 1 << 20) == _native.GH_ERR_INVALID
    its = ctypes.c_int32()
    x = np.zeros(4)
    assert lib.gh_cent_pagerank(None, 0.85, 100, 1e-6, _native.ptr(x), ctypes.byref(its)) == _native.GH_ERR_INVALID
    assert lib.gh_cent_paths(None, 0, None, None, None, None, None) == _native.GH_ERR_INVALID


def test_scales_follow_networkx():
    assert cent.betweenness_scale(2, True) is None
    assert cent.betweenness_scale(10, False) == 0.5
    assert cent.betweenness_scale(10, True) == 1 / (9 * 8)
    assert cent.betweenness_scale(10, True, k=5) == 1 / (9 * 8) * 10 / 5
    c = cent.closeness_from([1, 3, 5], [0, 3, 6], 5)
    assert c[0] == 0.0 and c[1] == (2 / 3) * (2 / 4) and c[2] == (4 / 6) * 1.0


SMALL = {
    "path": nx.path_graph(30),
    "star": nx.star_graph(40),
    "grid": nx.convert_node_labels_to_integers(nx.grid_2d_graph(7, 9)),
    "barbell": nx.barbell_graph(8, 5),
    "ba": nx.barabasi_albert_graph(200, 3, seed=1),
    "er_disconnected": nx.gnp_random_graph(150, 0.01, seed=2),
    "k12": nx.complete_graph(12),
}


@pytest.mark.parametrize("name", sorted(SMALL))
def test_restatement_matches_networkx(name):
    G = SMALL[name]
    n = G.number_of_nodes()
    edges = np.array(G.edges()).reshape(-1, 2)
    bc, ld, reached, dsum = ref.paths(n, edges, np.arange(n), batch=37)
    nb = nx.betweenness_centrality(G)
    nl = nx.load_centrality(G)
    nc = nx.closeness_centrality(G)
    np.testing.assert_allclose(bc * cent.betweenness_scale(n, True), [nb[i] for i in range(n)], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(ld / ((n - 1) * (n - 2)), [nl[i] for i in range(n)], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(cent.closeness_from(reached, dsum, n), [nc[i] for i in range(n)], rtol=1e-12, atol=0)
    x, its = ref.pagerank(n, edges)
    pr = nx.pagerank(G)
    np.testing.assert_allclose(x, [pr[i] for i in range(n)], rtol=1e-9, atol=1e-12)
    assert its > 0
    if its > 2:
        assert ref.pagerank(n, edges, max_iter=2)[1] == -1


def test_restatement_dependency_identity():
    # sum_v delta_s(v) = sum_v lambda_s(v) = sum_t (d(s, t) - 1) over the vertices t reached from s, t != s
    G = nx.barabasi_albert_graph(300, 2, seed=4)
    edges = np.array(G.edges())
    for s in (0, 17, 299):
        bc, ld, reached, dsum = ref.paths(300, edges, [s])
        want = dsum[0] - (reached[0] - 1)
        assert abs(bc.sum() - want) <= 1e-9 * want
        assert abs(ld.sum() - want) <= 1e-9 * want
