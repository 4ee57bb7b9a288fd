"""Cores and trusses without a GPU: the exported C ABI, the restatement (tests/cores_reference.py) against networkx on the
graphs of tests/test_hip_cores.py, and the Python layer of graphem-rapids_amd/cores.py and kshell_seed_selection over a
stand-in handle that answers from the restatement."""
import ctypes
import inspect
import os

import networkx as nx
import numpy as np
import pytest

import graphem_rapids_amd as gr
from graphem_rapids_amd import _native, cores

import cores_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CORE_SYMBOLS = ["gh_cent_cores", "gh_cent_truss"]
PUBLIC = ["core_number", "onion_layers", "degeneracy", "k_core", "k_shell", "k_crust", "k_corona", "truss_number", "k_truss"]


def test_core_symbols_declared_exported_and_listed():
    from graphem_rapids_amd import build as gra_build
    header = open(os.path.join(ROOT, "include", "graphem_hip.h")).read()
    assert header.index("graph statistics") < header.index("cores and trusses") < header.index("---- communities")
    gra_build.build()
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in CORE_SYMBOLS:
        assert name + "(" in header, name
        assert name in _native.SYMBOLS, name
        assert hasattr(lib, name), name
    assert len(_native.SIGNATURES["gh_cent_cores"][1]) == 4 and len(_native.SIGNATURES["gh_cent_truss"][1]) == 3


def test_null_handle_is_refused_without_a_device():
    lib = _native.load()
    rounds = ctypes.c_int32(7)
    out = np.zeros(4, dtype=np.int32)
    assert lib.gh_cent_cores(None, _native.ptr(out), _native.ptr(out), ctypes.byref(rounds)) == _native.GH_ERR_INVALID
    assert lib.gh_cent_last_error(None) == b"handle is NULL"
    assert lib.gh_cent_truss(None, _native.ptr(out), ctypes.byref(rounds)) == _native.GH_ERR_INVALID
    assert lib.gh_cent_last_error(None) == b"handle is NULL"


def test_public_names_are_exported():
    for name in PUBLIC:
        assert name in gr.__all__, name
        assert getattr(gr, name) is getattr(cores, name)
    assert "cores" in gr.__all__ and "kshell_seed_selection" in gr.__all__
    for name in ("core_layers", "truss_numbers"):
        assert callable(getattr(gr.CentralityGraph, name))
    for name in ("cores", "truss"):
        assert callable(getattr(_native.CentGraph, name))


def test_benchmark_functions_gained_only_false_keywords():
    for fn, new in ((gr.run_benchmark, "cores"), (gr.benchmark_correlations, "cores"), (gr.run_influence_benchmark, "kshell")):
        params = inspect.signature(fn).parameters
        assert params[new].default is False
        if fn is not gr.run_influence_benchmark:
            assert params[new].kind == inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(gr.run_influence_benchmark).parameters) == [
        "graph_generator", "graph_params", "k", "p", "iterations", "dim", "num_layout_iterations", "layout_params", "backend",
        "ris", "kshell"]
    keyword_only = [n for n, p in inspect.signature(gr.run_benchmark).parameters.items() if p.kind == inspect.Parameter.KEYWORD_ONLY]
    assert keyword_only == ["betweenness_k", "cores"]
    keyword_only = [n for n, p in inspect.signature(gr.benchmark_correlations).parameters.items()
                    if p.kind == inspect.Parameter.KEYWORD_ONLY]
    assert keyword_only == ["betweenness_k", "bootstrap_reps", "bootstrap_seed", "cores"]


# ---- the restatement equals networkx ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ref.VERTEX_GRAPHS)
def test_reference_peel_is_networkx(name):
    G, n, _ = ref.graph(name)
    core, layer, rounds = ref.peel_of(name)
    want_core, want_layer = nx.core_number(G), nx.onion_layers(G)
    assert core.tolist() == [want_core[v] for v in range(n)]
    assert layer.tolist() == [want_layer[v] for v in range(n)]
    assert rounds == (int(layer.max()) if n else 0)
    if name in ref.VERTEX_PINS:
        assert (n, G.number_of_edges(), int(core.max()), rounds) == ref.VERTEX_PINS[name]
    if name == "gnp2000":
        assert nx.number_connected_components(G) == 35 and len(np.unique(core)) == 4 and (core == 0).any()
    if name == "gnp600":
        assert len(np.unique(core)) == 5
    if name == "k20":
        assert (core == 19).all() and rounds == 1
    if name == "star300":
        assert (core == 1).all() and layer.tolist() == [2] + [1] * 299
    if name == "cycle101":
        assert (core == 2).all() and (layer == 1).all()
    if name == "isolated":
        assert core.sum() == 2 and core[17] == core[301] == 1 and layer[17] == layer[301] == 2 and np.sum(layer == 1) == 300


@pytest.mark.parametrize("name", ref.EDGE_GRAPHS)
def test_reference_truss_is_networkx_k_truss(name):
    G, n, _ = ref.graph(name)
    edges, truss, rounds = ref.truss_of(name)
    top = int(truss.max()) if len(truss) else 0
    assert (len(edges), top, rounds) == ref.EDGE_PINS[name]
    assert len(truss) == 0 or truss.min() >= 2
    for k in range(2, top + 2):
        H = nx.k_truss(G, k)
        assert np.array_equal(ref.canonical_edges(n, ref.edge_array(H)), edges[truss >= k]), k
    if name == "relaxed_caveman":
        assert len(np.unique(truss)) == 7
    if name == "k20":
        assert (truss == 20).all()


def test_messy_edges_give_the_same_peels():
    _, n, e = ref.graph("relaxed_caveman")
    m = ref.messy(n, e, seed=5)
    core, layer, rounds = ref.peel(n, m)
    want = ref.peel_of("relaxed_caveman")
    assert np.array_equal(core, want[0]) and np.array_equal(layer, want[1]) and rounds == want[2]
    edges, truss, rounds = ref.truss(n, m)
    want = ref.truss_of("relaxed_caveman")
    assert np.array_equal(edges, want[0]) and np.array_equal(truss, want[1]) and rounds == want[2]


# ---- the Python layer over a stand-in handle -------------------------------------------------------------------------
class _ReferenceHandle:
    """What _native.CentGraph offers cores.py, answered by the restatement."""
    built = 0

    def __init__(self, n, edges, device_id=0):
        del device_id
        type(self).built += 1
        self.n, self.e = int(n), np.asarray(edges, dtype=np.int64).reshape(-1, 2)

    def cores(self):
        return ref.peel(self.n, self.e)

    def truss(self):
        _, truss, rounds = ref.truss(self.n, self.e)
        return truss, rounds

    def close(self):
        pass


@pytest.fixture
def host_only(monkeypatch):
    monkeypatch.setattr(_native, "CentGraph", _ReferenceHandle)
    _ReferenceHandle.built = 0


def _same_subgraph(got, H, nodes=None):
    """got = (adjacency, vertices) of ours; H networkx's subgraph: the same vertices, ascending in the original order,
    and the same edges between them."""
    adjacency, vertices = got
    vertices = list(vertices)
    order = list(nodes) if nodes is not None else None
    want = sorted(H.nodes(), key=(order.index if order is not None else None))
    assert vertices == want
    assert adjacency.shape == (len(want), len(want))
    assert (adjacency != adjacency.T).nnz == 0 and (adjacency.nnz == 0 or (adjacency.data == 1).all())
    coo = adjacency.tocoo()
    ours = {frozenset((vertices[i], vertices[j])) for i, j in zip(coo.row.tolist(), coo.col.tolist())}
    assert ours == {frozenset(e) for e in H.edges()}
    assert adjacency.nnz == 2 * H.number_of_edges()


SUBGRAPH_GRAPHS = {
    "gnp2000": lambda: ref.graph("gnp2000")[0],
    "relaxed_caveman": lambda: ref.graph("relaxed_caveman")[0],
    "ba1000": lambda: ref.graph("ba1000")[0],
    "path_plus_triangle": lambda: nx.Graph([(0, 1), (1, 2), (2, 0), (2, 3), (3, 4), (6, 7)]),
}


@pytest.mark.parametrize("name", sorted(SUBGRAPH_GRAPHS))
def test_core_subgraphs_are_networkx(host_only, name):
    G = SUBGRAPH_GRAPHS[name]()
    top = max(nx.core_number(G).values())
    assert gr.core_number(G) == nx.core_number(G) and gr.onion_layers(G) == nx.onion_layers(G)
    assert all(type(x) is int for x in gr.core_number(G).values())   # pylint: disable=unidiomatic-typecheck
    assert gr.degeneracy(G) == top
    for fn in ("k_core", "k_shell", "k_crust"):
        for k in [None, 0, 1, 2, top, top + 1]:
            _same_subgraph(getattr(gr, fn)(G, k, return_vertices=True), getattr(nx, fn)(G, k))
    for k in [0, 1, 2, top]:
        _same_subgraph(gr.k_corona(G, k, return_vertices=True), nx.k_corona(G, k))
    plain = gr.k_core(G)
    assert plain.shape[0] == nx.k_core(G).number_of_nodes() and plain.dtype == gr.edges_to_adjacency(2, [[0, 1]]).dtype


def test_truss_subgraphs_are_networkx(host_only):
    G = ref.graph("relaxed_caveman")[0]
    t = gr.truss_number(G)
    edges, truss, _ = ref.truss_of("relaxed_caveman")
    assert list(t) == [tuple(e) for e in edges.tolist()] and list(t.values()) == truss.tolist()
    assert all(type(x) is int for x in t.values())   # pylint: disable=unidiomatic-typecheck
    for k in [0, 2, 3, 5, 9, 10]:
        _same_subgraph(gr.k_truss(G, k, return_vertices=True), nx.k_truss(G, k))
    assert gr.k_truss(G, 10).shape == (0, 0)


def test_labelled_graphs_are_keyed_by_node(host_only):
    B = nx.barbell_graph(5, 2)
    names = {i: f"v{(7 * i) % 12}" for i in range(12)}   # not in sorted order
    G = nx.relabel_nodes(B, names)
    nodes = list(G.nodes())
    assert gr.core_number(G) == nx.core_number(G) and gr.onion_layers(G) == nx.onion_layers(G)
    assert list(gr.core_number(G)) == nodes
    for k in (None, 1, 4):
        _same_subgraph(gr.k_core(G, k, return_vertices=True), nx.k_core(G, k), nodes)
        _same_subgraph(gr.k_shell(G, k, return_vertices=True), nx.k_shell(G, k), nodes)
        _same_subgraph(gr.k_crust(G, k, return_vertices=True), nx.k_crust(G, k), nodes)
    _same_subgraph(gr.k_corona(G, 4, return_vertices=True), nx.k_corona(G, 4), nodes)
    _same_subgraph(gr.k_truss(G, 5, return_vertices=True), nx.k_truss(G, 5), nodes)
    t = gr.truss_number(G)
    edges, truss, _ = ref.truss(12, ref.edge_array(B))
    assert list(t) == [(names[u], names[v]) for u, v in edges.tolist()] and list(t.values()) == truss.tolist()
    assert sorted(set(t.values())) == [2, 5] and t[(names[4], names[5])] == 2
    assert gr.kshell_seed_selection(G, 3) == [names[i] for i in _kshell_order(12, ref.edge_array(B))[:3]]


def test_other_inputs(host_only):
    G = ref.graph("ba1000")[0]
    want = nx.core_number(G)
    e = ref.edge_array(G)
    assert gr.core_number(e) == want
    assert gr.core_number(gr.edges_to_adjacency(1000, e)) == want
    g = gr.CentralityGraph(G)
    assert gr.core_number(g) == want and gr.onion_layers(g) == nx.onion_layers(G)
    core, layer = g.core_layers()
    assert core.dtype == layer.dtype == np.int32 and core.shape == layer.shape == (1000,)
    t = g.truss_numbers()
    assert t.dtype == np.int32 and t.shape == (len(g.edges),)
    g.close()
    loops = np.concatenate([e, [[3, 3], [9, 9]]])   # arrays drop self-loops silently
    assert gr.core_number(loops) == want and gr.onion_layers(loops) == nx.onion_layers(G)
    with pytest.raises(NotImplementedError):
        gr.core_number(nx.DiGraph([(0, 1)]))
    with pytest.raises(NotImplementedError):
        gr.k_truss(nx.MultiGraph([(0, 1)]), 3)


def test_null_graph(host_only):
    G = nx.Graph()
    assert gr.core_number(G) == {} and gr.onion_layers(G) == {} and gr.truss_number(G) == {} and gr.degeneracy(G) == 0
    assert gr.k_core(G, 1).shape == (0, 0) and gr.k_truss(G, 3).shape == (0, 0)
    with pytest.raises(ValueError):   # networkx: max() of no core numbers
        nx.k_core(G)
    with pytest.raises(ValueError):
        gr.k_core(G)
    g = gr.CentralityGraph(np.zeros((0, 2), dtype=np.int64))
    core, layer = g.core_layers()
    assert core.shape == layer.shape == (0,) and core.dtype == layer.dtype == np.int32
    assert g.truss_numbers().shape == (0,) and g.truss_numbers().dtype == np.int32
    assert gr.kshell_seed_selection(G, 0) == []
    assert _ReferenceHandle.built == 0


def test_self_loops_raise_networkx_messages_before_a_handle_exists(host_only):
    G = nx.Graph([(0, 1), (1, 2), (2, 0), (1, 1)])
    calls = [(nx.core_number, gr.core_number, ()), (nx.onion_layers, gr.onion_layers, ()), (nx.k_truss, gr.k_truss, (3,)),
             (nx.k_core, gr.k_core, ()), (nx.k_shell, gr.k_shell, ()), (nx.k_crust, gr.k_crust, ()), (nx.k_corona, gr.k_corona, (1,))]
    for theirs, ours, args in calls:
        with pytest.raises(nx.NetworkXNotImplemented) as want:
            theirs(G, *args)
        with pytest.raises(nx.NetworkXNotImplemented) as got:
            ours(G, *args)
        assert str(got.value) == str(want.value), ours.__name__
    with pytest.raises(nx.NetworkXNotImplemented) as a:
        nx.core_number(G)
    with pytest.raises(nx.NetworkXNotImplemented) as b:
        nx.onion_layers(G)
    assert str(a.value) != str(b.value)   # two messages, each copied
    for fn in (gr.truss_number, gr.degeneracy):
        with pytest.raises(nx.NetworkXNotImplemented):
            fn(G)
    assert _ReferenceHandle.built == 0


def test_precomputed_core_number_skips_the_pass(host_only, monkeypatch):
    G = ref.graph("relaxed_caveman")[0]
    want = nx.core_number(G)
    monkeypatch.setattr(_ReferenceHandle, "cores", lambda self: pytest.fail("the device pass ran"))
    as_array = np.array([want[v] for v in range(G.number_of_nodes())])
    for given in (want, as_array):
        for fn in ("k_core", "k_shell", "k_crust"):
            for k in (None, 5):
                _same_subgraph(getattr(gr, fn)(G, k, core_number=given, return_vertices=True), getattr(nx, fn)(G, k, want))
        _same_subgraph(gr.k_corona(G, 8, core_number=given, return_vertices=True), nx.k_corona(G, 8, want))
    with pytest.raises(ValueError):
        gr.k_core(G, 3, core_number=as_array[:-1])
    # a made-up table is used as given, as in networkx
    fake = {v: v % 4 for v in G}
    _same_subgraph(gr.k_shell(G, 2, core_number=fake, return_vertices=True), nx.k_shell(G, 2, fake))


# ---- k-shell seeds ---------------------------------------------------------------------------------------------------
def _kshell_order(n, edges):
    core, layer, _ = ref.peel(n, edges)
    deg = np.bincount(ref.canonical_edges(n, edges).ravel(), minlength=n)
    return sorted(range(n), key=lambda v: (-core[v], -layer[v], -deg[v], v))


@pytest.mark.parametrize("name", ["gnp2000", "ba1000", "lollipop", "star300"])
def test_kshell_seed_order_and_bounds(host_only, name):
    G, n, e = ref.graph(name)
    order = _kshell_order(n, e)
    for k in (0, 1, 7, n):
        assert gr.kshell_seed_selection(G, k) == order[:k]
    assert gr.kshell_seed_selection(e, 5) == order[:5] == gr.kshell_seed_selection(G, 5)   # a pure function of the graph
    core = nx.core_number(G)
    seeds = gr.kshell_seed_selection(G, 20)
    assert [core[v] for v in seeds] == sorted((core[v] for v in seeds), reverse=True)
    assert core[seeds[0]] == max(core.values())
    for bad in (-1, n + 1):
        with pytest.raises(ValueError):
            gr.kshell_seed_selection(G, bad)
