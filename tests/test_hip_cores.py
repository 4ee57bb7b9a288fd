"""gh_cent_cores / gh_cent_truss (csrc/cores.hip) and graphem-rapids_amd/cores.py against the restatement
(tests/cores_reference.py) array for array, round counts included, against networkx, against the values pinned for the
graphs, and against themselves (edge order, duplicates, self-loops, repeated calls, other calls on the handle in between).
Everything is an integer, so every comparison is exact."""
import ctypes

import networkx as nx
import numpy as np
import pytest
from scipy import stats

import graphem_rapids_amd as gr
from graphem_rapids_amd import _native, influence

import cores_reference as ref

pytestmark = pytest.mark.gpu


def _cores(n, edges):
    """(core, layer, rounds) from a fresh handle over an edge array."""
    g = gr.CentralityGraph(edges, n=n)
    try:
        if n == 0:
            return g.core_layers() + (0,)
        return g._g.cores()   # pylint: disable=protected-access
    finally:
        g.close()


def _truss(n, edges):
    """(canonical edges, truss, rounds) from a fresh handle over an edge array."""
    g = gr.CentralityGraph(edges, n=n)
    try:
        return (g.edges,) + g._g.truss()   # pylint: disable=protected-access
    finally:
        g.close()


def _same(got, want):
    return got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want)


# ---- vertex peel -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ref.VERTEX_GRAPHS)
def test_vertex_peel_is_the_restatement_and_networkx(name):
    G, n, e = ref.graph(name)
    core, layer, rounds = _cores(n, e)
    want_core, want_layer, want_rounds = ref.peel_of(name)
    assert _same(core, want_core) and _same(layer, want_layer) and rounds == want_rounds
    theirs_core, theirs_layer = nx.core_number(G), nx.onion_layers(G)
    assert core.tolist() == [theirs_core[v] for v in range(n)]
    assert layer.tolist() == [theirs_layer[v] for v in range(n)]
    assert rounds == (int(layer.max()) if n else 0)
    if name in ref.VERTEX_PINS:
        assert (n, G.number_of_edges(), int(core.max()), rounds) == ref.VERTEX_PINS[name]
    if name == "k20":
        assert (core == 19).all() and (layer == 1).all()
    if name == "star300":
        assert (core == 1).all() and layer.tolist() == [2] + [1] * 299
    if name == "isolated":
        assert np.sum(core) == 2 and np.sum(layer == 1) == 300 and layer[17] == layer[301] == 2


# ---- edge peel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ref.EDGE_GRAPHS)
def test_edge_peel_is_the_restatement_and_networkx(name):
    G, n, e = ref.graph(name)
    edges, truss, rounds = _truss(n, e)
    want_edges, want_truss, want_rounds = ref.truss_of(name)
    assert np.array_equal(edges, want_edges)
    assert _same(truss, want_truss) and rounds == want_rounds
    top = int(truss.max()) if len(truss) else 0
    assert (len(edges), top, rounds) == ref.EDGE_PINS[name]
    for k in sorted({2, 3, top}):
        H = nx.k_truss(G, k)
        assert np.array_equal(ref.canonical_edges(n, ref.edge_array(H)), edges[truss >= k]), k


# ---- a pure function of the edge set ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gnp2000", "lollipop", "gnp600", "relaxed_caveman"])
def test_vertex_peel_ignores_order_duplicates_and_self_loops(name):
    _, n, e = ref.graph(name)
    core, layer, rounds = _cores(n, ref.messy(n, e, seed=11))
    want = ref.peel_of(name)
    assert _same(core, want[0]) and _same(layer, want[1]) and rounds == want[2]


@pytest.mark.parametrize("name", ["relaxed_caveman", "plc3000", "wheel5001", "barbell"])
def test_edge_peel_ignores_order_duplicates_and_self_loops(name):
    _, n, e = ref.graph(name)
    edges, truss, rounds = _truss(n, ref.messy(n, e, seed=12))
    want = ref.truss_of(name)
    assert np.array_equal(edges, want[0]) and _same(truss, want[1]) and rounds == want[2]


@pytest.mark.parametrize("name", ["relaxed_caveman", "gnp600"])
def test_repeated_calls_and_other_calls_in_between(name):
    _, n, e = ref.graph(name)
    want_core, want_layer, want_rounds = ref.peel_of(name)
    _, want_truss, want_truss_rounds = ref.truss_of(name)
    g = gr.CentralityGraph(e, n=n)
    before = _native.live_allocations()

    def check():
        core, layer, rounds = g._g.cores()   # pylint: disable=protected-access
        assert _same(core, want_core) and _same(layer, want_layer) and rounds == want_rounds
        truss, rounds = g._g.truss()   # pylint: disable=protected-access
        assert _same(truss, want_truss) and rounds == want_truss_rounds
        assert _native.live_allocations() == before   # all device state is released on return
    check()
    check()
    labels = g.component_labels()
    triangles = g.triangle_counts()
    g.louvain_levels(seed=1)
    check()
    assert np.array_equal(g.component_labels(), labels) and np.array_equal(g.triangle_counts(), triangles)
    core, layer = g.core_layers()
    assert _same(core, want_core) and _same(layer, want_layer) and _same(g.truss_numbers(), want_truss)
    g.close()


def test_either_output_may_be_null():
    _, n, e = ref.graph("gnp2000")
    want_core, want_layer, want_rounds = ref.peel_of("gnp2000")
    g = gr.CentralityGraph(e, n=n)
    h = g._g   # pylint: disable=protected-access
    core, layer = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    rounds = ctypes.c_int32(0)
    assert h.lib.gh_cent_cores(h.handle, _native.ptr(core), None, ctypes.byref(rounds)) == _native.GH_OK
    assert np.array_equal(core, want_core) and rounds.value == want_rounds
    assert h.lib.gh_cent_cores(h.handle, None, _native.ptr(layer), None) == _native.GH_OK
    assert np.array_equal(layer, want_layer)
    assert h.lib.gh_cent_cores(h.handle, None, None, ctypes.byref(rounds)) == _native.GH_OK and rounds.value == want_rounds
    with pytest.raises(ValueError, match="truss must not be NULL"):
        h._raise(h.lib.gh_cent_truss(h.handle, None, ctypes.byref(rounds)))   # pylint: disable=protected-access
    g.close()
    # no edges: nothing to peel, zero rounds
    g = gr.CentralityGraph(np.zeros((0, 2), dtype=np.int64), n=5)
    truss, rounds = g._g.truss()   # pylint: disable=protected-access
    assert truss.shape == (0,) and rounds == 0
    core, layer, rounds = g._g.cores()   # pylint: disable=protected-access
    assert not core.any() and (layer == 1).all() and rounds == 1
    g.close()


# ---- the Python layer ------------------------------------------------------------------------------------------------
def _same_subgraph(got, H, nodes):
    adjacency, vertices = got
    vertices = list(vertices)
    assert vertices == sorted(H.nodes(), key=nodes.index)
    coo = adjacency.tocoo()
    assert {frozenset((vertices[i], vertices[j])) for i, j in zip(coo.row.tolist(), coo.col.tolist())} == \
        {frozenset(e) for e in H.edges()}
    assert adjacency.shape == (len(vertices),) * 2 and adjacency.nnz == 2 * H.number_of_edges()


def test_results_are_keyed_by_node():
    G = ref.graph("barbell")[0]
    nodes = list(G.nodes())
    assert nodes != list(range(len(nodes)))   # barbell_graph lists the path's vertex last
    assert gr.core_number(G) == nx.core_number(G) and list(gr.core_number(G)) == nodes
    assert gr.onion_layers(G) == nx.onion_layers(G)
    assert gr.degeneracy(G) == 19
    t = gr.truss_number(G)
    assert {frozenset(e) for e in t} == {frozenset(e) for e in G.edges()}
    assert all(nodes.index(u) < nodes.index(v) for u, v in t)
    assert {frozenset(e) for e, value in t.items() if value >= 20} == {frozenset(e) for e in nx.k_truss(G, 20).edges()}
    assert sorted(set(t.values())) == [2, 20]
    for k in (None, 1, 19):
        _same_subgraph(gr.k_core(G, k, return_vertices=True), nx.k_core(G, k), nodes)
        _same_subgraph(gr.k_shell(G, k, return_vertices=True), nx.k_shell(G, k), nodes)
        _same_subgraph(gr.k_crust(G, k, return_vertices=True), nx.k_crust(G, k), nodes)
    _same_subgraph(gr.k_corona(G, 19, return_vertices=True), nx.k_corona(G, 19), nodes)
    _same_subgraph(gr.k_truss(G, 3, return_vertices=True), nx.k_truss(G, 3), nodes)
    with pytest.raises(nx.NetworkXNotImplemented, match="Input graph contains self loops"):
        gr.onion_layers(nx.Graph([(0, 1), (1, 1)]))


def _generator(n):
    return ref.edge_array(nx.gnp_random_graph(n, 0.03, seed=5))


def test_benchmark_correlations_with_cores():
    kw = dict(num_iterations=5, sample_size=64, n_neighbors=5, seed=0)
    plain = gr.benchmark_correlations(_generator, {"n": 300}, **kw)
    res = gr.benchmark_correlations(_generator, {"n": 300}, cores=True, bootstrap_reps=20, **kw)
    new = {"core_number", "onion_layer"}
    assert set(res) == set(plain) | new and not new & set(plain)
    assert set(res["correlations"]) == set(plain["correlations"]) | new and not new & set(plain["correlations"])
    core, layer, _ = ref.peel(300, _generator(300))
    for name, want in (("core_number", core), ("onion_layer", layer)):
        assert res[name].dtype == np.float64 and np.array_equal(res[name], want)
        rho, p = stats.spearmanr(res["radii"], res[name])
        entry = res["correlations"][name]
        assert set(entry) == {"rho", "p", "ci_low", "ci_high"} and entry["ci_low"] <= entry["ci_high"]
        assert (entry["rho"], entry["p"]) == (rho, p)
    assert len(np.unique(layer)) > len(np.unique(core)) > 1   # the finer of the two
    for name in plain["correlations"]:
        assert set(plain["correlations"][name]) == {"rho", "p"}
        assert set(res["correlations"][name]) == {"rho", "p", "ci_low", "ci_high"}
    assert np.array_equal(res["degree"], plain["degree"])


def test_run_influence_benchmark_with_kshell(monkeypatch):
    monkeypatch.setattr(influence, "_draw_seed", lambda seed: 1234 if seed is None else int(seed))   # every coin seed fixed
    params = {"n": 200, "communities": 4, "deg_in": 6, "deg_out": 1}
    kw = dict(k=5, p=0.1, iterations=20, num_layout_iterations=3)
    plain = gr.run_influence_benchmark(gr.planted_partition_edges, params, **kw)
    res = gr.run_influence_benchmark(gr.planted_partition_edges, params, kshell=True, **kw)
    extra = {"kshell_seeds", "kshell_influence", "kshell_time"}
    assert set(res) == set(plain) | extra and not extra & set(plain)
    edges = gr.planted_partition_edges(**params)
    graph = gr.InfluenceGraph(edges, n=200)
    assert res["kshell_seeds"] == gr.kshell_seed_selection(graph, 5) == gr.kshell_seed_selection(edges, 5)
    core, layer, _ = ref.peel(200, edges)
    deg = np.bincount(ref.canonical_edges(200, edges).ravel(), minlength=200)
    assert res["kshell_seeds"] == sorted(range(200), key=lambda v: (-core[v], -layer[v], -deg[v], v))[:5]
    assert res["kshell_influence"] == gr.ndlib_estimated_influence(graph, res["kshell_seeds"], 0.1, 20, seed=1234)[0]
    assert 5 <= res["kshell_influence"] <= 200
    graph.close()
