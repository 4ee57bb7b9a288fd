"""Communities without a GPU: the exported C ABI, the numpy restatement of the Louvain rule (tests/communities_reference.py)
against networkx -- modularity values, planted partitions, quality beside networkx's Louvain, the rule's invariants and
edge cases -- and the Python layer of graphem-rapids_amd/communities.py over a stand-in handle that answers from the
restatement."""
import ctypes
import functools
import os

import networkx as nx
import numpy as np
import pytest
from networkx.algorithms.community.quality import NotAPartition

import graphem_rapids_amd as gr
from graphem_rapids_amd import _native, communities

import communities_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COMMUNITY_SYMBOLS = ["gh_cent_modularity", "gh_cent_louvain"]
PUBLIC = ["modularity", "louvain_communities", "louvain_partitions", "community_labels", "adjusted_rand_index"]


def test_community_symbols_declared_exported_and_listed():
    from graphem_rapids_amd import build as gra_build
    header = open(os.path.join(ROOT, "include", "graphem_hip.h")).read()
    assert "communities: Louvain levels and exact modularity" in header
    gra_build.build()
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in COMMUNITY_SYMBOLS:
        assert name + "(" in header, name
        assert name in _native.SYMBOLS, name
        assert hasattr(lib, name), name


def test_public_names_are_exported():
    for name in PUBLIC:
        assert name in gr.__all__, name
        assert getattr(gr, name) is getattr(communities, name)
    for name in ("louvain_levels", "modularity_terms"):
        assert callable(getattr(gr.CentralityGraph, name))
    for name in ("louvain", "modularity"):
        assert callable(getattr(_native.CentGraph, name))


# ---- the restatement, computed once per graph ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _graphs():
    out = {name: (n, e) for name, (n, e, _) in ref.planted().items()}
    out.update(ref.quality_graphs())
    out.update(ref.edge_cases())
    return out


@functools.lru_cache(maxsize=None)
def _run(name, seed=0):
    n, e = _graphs()[name]
    trails = []
    labels, numerators, counts, rounds, M = ref.louvain(n, e, seed=seed, trails=trails)
    labels.setflags(write=False)
    return labels, numerators, counts, rounds, M, trails


def _nx_graph(name):
    n, e = _graphs()[name]
    G = nx.empty_graph(n)
    G.add_edges_from(np.asarray(e).tolist())
    return G


def _sets(labels):
    return [set(np.flatnonzero(labels == v).tolist()) for v in np.unique(labels)]


PLANTED = ["sbm8", "sbm6", "caveman", "relaxed"]
QUALITY = ["gnp3000", "ba3000", "ws2000", "road40", "tree2_9", "regular2000"]


@pytest.mark.parametrize("name", PLANTED)
def test_modularity_value_is_networkx(name):
    """N / M^2 against nx.community.modularity: the two differ only in float summation order."""
    n, e, want = ref.planted()[name]
    G = _nx_graph(name)
    rng = np.random.default_rng(11)
    labellings = [want] + [rng.integers(0, rng.integers(1, 40), size=n) for _ in range(5)]
    for labels in labellings:
        ours = ref.q_of(ref.modularity_terms(n, e, labels))
        theirs = nx.community.modularity(G, _sets(labels))
        print(name, ours, theirs)
        assert abs(ours - theirs) <= 1e-12


@pytest.mark.parametrize("name", PLANTED)
def test_planted_structure_is_recovered_exactly(name):
    want = ref.planted()[name][2]
    labels = _run(name)[0]
    assert gr.adjusted_rand_index(labels[-1], want) == 1.0
    assert np.array_equal(labels[-1], want)   # both are min-id labels


@pytest.mark.parametrize("name", QUALITY)
def test_quality_against_networkx_louvain(name):
    """Final Q >= 0.98 x the smallest Q of networkx's Louvain over seeds 0 .. 4 (DESIGN.md section 18 has the values)."""
    _, numerators, _, _, M, _ = _run(name)
    ours = numerators[-1] / (M * M)
    G = _nx_graph(name)
    theirs = [nx.community.modularity(G, nx.community.louvain_communities(G, seed=s)) for s in range(5)]
    print(name, "ours %.4f networkx %.4f .. %.4f" % (ours, min(theirs), max(theirs)))
    assert ours >= 0.98 * min(theirs)


@pytest.mark.parametrize("name", PLANTED + QUALITY)
def test_invariants(name):
    n, e = _graphs()[name]
    labels, numerators, counts, _, M, trails = _run(name)
    flat = [N for trail in trails for N in trail]
    assert all(a < b for a, b in zip(flat, flat[1:])), "numerators rise over accepted rounds and levels"
    assert [trail[-1] for trail in trails] == numerators
    for l, row in enumerate(labels):
        assert np.array_equal(row, ref.min_member_labels(np.unique(row, return_inverse=True)[1].reshape(n)))
        assert len(np.unique(row)) == counts[l]
        sI, sT2, M2 = ref.modularity_terms(n, e, row)
        assert (M2 * sI - sT2, M2) == (numerators[l], M)
        if l + 1 < len(labels):   # every community of this level lies inside one of the next
            assert len(np.unique(np.column_stack([row, labels[l + 1]]), axis=0)) == counts[l]
            assert counts[l + 1] < counts[l]


def test_seed_changes_the_partition_and_the_same_seed_does_not():
    a, b = _run("gnp3000")[0][-1], _run("gnp3000", seed=1)[0][-1]
    assert not np.array_equal(a, b)
    n, e = _graphs()["gnp3000"]
    again = ref.louvain(n, e[np.random.default_rng(2).permutation(len(e))], seed=0)[0][-1]
    assert np.array_equal(a, again)


def test_edge_cases():
    def final(name):
        labels, numerators, counts, _, M, _ = _run(name)
        return labels[-1].tolist(), counts[-1], numerators[-1], M

    assert final("n1") == ([0], 1, 0, 0)
    assert final("n2") == ([0, 0], 1, 0, 2)
    assert final("no_edges") == (list(range(7)), 7, 0, 0)
    assert final("triangle_isolated") == ([0, 1, 1, 3, 1], 3, 0, 6)
    labels, count, N, M = final("two_triangles")
    assert (labels, count) == ([0, 0, 0, 3, 3, 3], 2) and N * 14 == 5 * M * M   # Q = 5 / 14
    for name in ("k20", "k8_12"):   # ties everywhere; no partition of either has Q > 0
        assert final(name)[2] == 0, name
    assert final("k20")[1] == 1
    labels, count, N, _ = final("star200")
    assert (count, N) == (1, 0) and not any(labels)


# ---- partition agreement ---------------------------------------------------------------------------------------------
def test_adjusted_rand_index_is_the_pair_count():
    rng = np.random.default_rng(5)
    for n in (0, 1, 2, 3, 7, 30, 60):
        for _ in range(6):
            a, b = rng.integers(0, rng.integers(1, 6), size=n), rng.integers(0, rng.integers(1, 6), size=n)
            assert abs(gr.adjusted_rand_index(a, b) - ref.pair_count_ari(a, b)) <= 1e-15
    ones, singles = np.zeros(9, dtype=int), np.arange(9)
    assert gr.adjusted_rand_index(ones, ones + 4) == 1.0 and gr.adjusted_rand_index(singles, singles[::-1]) == 1.0
    assert gr.adjusted_rand_index(ones, singles) == 0.0
    assert gr.adjusted_rand_index(["a", "a", "b"], [2, 2, 7]) == 1.0
    with pytest.raises(ValueError):
        gr.adjusted_rand_index([0, 1], [0])


# ---- host-side argument checks (nothing here reaches the device) -----------------------------------------------------
def test_weight_and_resolution_are_refused():
    G = nx.path_graph(4)
    for fn in (gr.louvain_communities, gr.louvain_partitions):
        with pytest.raises(NotImplementedError):
            fn(G, weight="weight")
        with pytest.raises(NotImplementedError):
            fn(G, resolution=1.5)
        with pytest.raises(ValueError, match="max_level argument must be a positive integer or None"):
            fn(gr.CentralityGraph(np.zeros((0, 2), dtype=np.int64)), max_level=0)
    with pytest.raises(NotImplementedError):
        gr.modularity(G, [{0, 1}, {2, 3}], weight="weight")
    with pytest.raises(NotImplementedError):
        gr.modularity(G, [{0, 1}, {2, 3}], resolution=2)


def test_null_graph():
    g = gr.CentralityGraph(np.zeros((0, 2), dtype=np.int64))
    assert gr.louvain_communities(g) == nx.community.louvain_communities(nx.Graph(), seed=0) == []
    assert gr.louvain_partitions(g) == [] and gr.community_labels(g).shape == (0,)
    assert g.louvain_levels()[0].shape == (0, 0) and g.modularity_terms([]) == (0, 0, 0)
    with pytest.raises(ZeroDivisionError):
        gr.modularity(g, [])
    with pytest.raises(ValueError):
        g.modularity_terms([0])
    with pytest.raises(ValueError):
        g.louvain_levels(max_levels=0)


# ---- the Python layer over a stand-in handle -------------------------------------------------------------------------
class _ReferenceHandle:
    """What _native.CentGraph offers the communities, answered by the restatement."""

    def __init__(self, n, edges, device_id=0):
        del device_id
        self.n, self.e = int(n), np.asarray(edges, dtype=np.int64).reshape(-1, 2)

    def louvain(self, seed=0, max_levels=32, max_rounds=1000):
        labels, numerators, counts, rounds, M = ref.louvain(self.n, self.e, seed, max_levels, max_rounds)
        return labels, numerators, np.array(counts, dtype=np.int64), np.array(rounds, dtype=np.int32), M

    def modularity(self, labels):
        return ref.modularity_terms(self.n, self.e, labels)

    def close(self):
        pass


@pytest.fixture
def host_only(monkeypatch):
    monkeypatch.setattr(_native, "CentGraph", _ReferenceHandle)


def test_python_layer_on_labelled_nodes(host_only):
    G = nx.relabel_nodes(nx.barbell_graph(6, 0), {i: f"v{i}" for i in range(12)})
    left, right = {f"v{i}" for i in range(6)}, {f"v{i}" for i in range(6, 12)}
    assert gr.louvain_communities(G) == [left, right]
    parts = gr.louvain_partitions(G)
    assert parts[-1] == [left, right] and all(sum(len(c) for c in p) == 12 for p in parts)
    assert gr.louvain_communities(G, max_level=1) == parts[0]
    assert gr.community_labels(G).tolist() == [0] * 6 + [6] * 6 and gr.community_labels(G).dtype == np.int32
    assert gr.community_labels(G, level=0).tolist() == gr.CentralityGraph(G).louvain_levels()[0][0].tolist()
    for part in ([left, right], [{v} for v in G], [set(G)], iter([right, left]), [left, set(), right]):
        part = list(part)
        assert abs(gr.modularity(G, part) - nx.community.modularity(G, part)) <= 1e-12
    assert gr.modularity(G, np.array([3] * 6 + [9] * 6)) == gr.modularity(G, [left, right])
    assert gr.louvain_communities(G, threshold=1e-7, seed=None) == [left, right]


def test_not_a_partition(host_only):
    G = nx.path_graph(4)
    for bad in ([{0, 1}], [{0, 1}, {1, 2, 3}], [{0, 1}, {2, 3, 4}], [{0, 1}, {2}, {3}, {3}]):
        with pytest.raises(NotAPartition):
            nx.community.modularity(G, bad)
        with pytest.raises(NotAPartition):
            gr.modularity(G, bad)
    with pytest.raises(NotAPartition):
        gr.modularity(G, np.array([0, 1, 2]))
    with pytest.raises(ZeroDivisionError):
        nx.community.modularity(nx.empty_graph(3), [{0}, {1}, {2}])
    with pytest.raises(ZeroDivisionError):
        gr.modularity(nx.empty_graph(3), [{0}, {1}, {2}])


def test_edge_arrays_and_a_kept_handle(host_only):
    n, e, want = ref.planted()["caveman"]
    g = gr.CentralityGraph(e, n=n)
    labels, numerators, counts, rounds, M = g.louvain_levels()
    assert np.array_equal(labels[-1], want) and counts[-1] == 10 and M == 2 * len(e)
    assert g.modularity_terms(want) == ref.modularity_terms(n, e, want)
    assert gr.modularity(g, want) == numerators[-1] / (M * M) == 0.9
    assert gr.louvain_communities(e) == [set(range(10 * i, 10 * i + 10)) for i in range(10)]
    assert gr.adjusted_rand_index(gr.community_labels(g), want) == 1.0
    assert len(rounds) == len(labels)
