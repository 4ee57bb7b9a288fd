"""gh_cent_louvain / gh_cent_modularity (csrc/communities.hip) and graphem-rapids_amd/communities.py against the numpy
restatement of the rule (tests/communities_reference.py), id for id at every level, and against itself (identical
integers across edge order, duplicates, self-loops, memory budgets and repeated calls).  Every expected value is an
integer, so every comparison is exact.  The shapes are the smallest that reach each kernel: rows on both sides of the
short / long threshold, a row that overflows the LDS table, coarse levels with weights and self weights."""
import functools

import numpy as np
import pytest

import graphem_rapids_amd as gr
from graphem_rapids_amd import _native

import communities_reference as ref

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _graphs():
    out = dict(ref.edge_cases())
    out.update({name: (n, e) for name, (n, e, _) in ref.planted().items()})
    quality = ref.quality_graphs()
    out.update({name: quality[name] for name in ("gnp3000", "road40")})
    out["ladder"] = ref.degree_ladder()
    out["ring4096"] = ref.ring(4096)
    return out


@functools.lru_cache(maxsize=None)
def _want(name, seed=0):
    n, e = _graphs()[name]
    labels, numerators, counts, rounds, M = ref.louvain(n, e, seed=seed)
    labels.setflags(write=False)
    return labels, numerators, counts, rounds, M


def _same(got, want):
    labels, numerators, counts, rounds, M = got
    assert labels.dtype == np.int32 and labels.shape == want[0].shape
    assert np.array_equal(labels, want[0])
    assert (numerators, counts.tolist(), rounds.tolist(), M) == (want[1], want[2], want[3], want[4])


CASES = ["n1", "n2", "no_edges", "triangle_isolated", "two_triangles", "k20", "k8_12", "star200", "sbm8", "sbm6", "caveman",
         "relaxed", "gnp3000", "road40", "ladder", "ring4096"]


@pytest.mark.parametrize("name", CASES)
def test_levels_equal_the_restatement(name):
    n, e = _graphs()[name]
    g = gr.CentralityGraph(e, n=n)
    got = g.louvain_levels()
    g.close()
    _same(got, _want(name))


def test_the_cases_reach_every_path():
    """What the list above is for: coarse levels (weights in the thousands, self weights), both row kernels, the spill."""
    assert len(_want("road40")[0]) >= 4 and len(_want("gnp3000")[0]) >= 3
    n, e = _graphs()["ladder"]
    assert n < 20000
    deg = np.bincount(e.ravel(), minlength=n)
    assert set(ref.LADDER_DEGREES) <= set(deg.tolist()) and (deg == 5000).sum() == 2
    first = _want("ladder")[0][0]
    hub = n - 5001
    assert len(np.unique(first[e[(e == hub).any(axis=1)].max(axis=1)])) > 1024   # communities in the hub's row > LDS slots


@pytest.mark.parametrize("name", ["gnp3000", "ladder"])
def test_invariance_bit_for_bit(name):
    n, e = _graphs()[name]
    want = _want(name)
    g = gr.CentralityGraph(ref.messy(n, e, seed=3), n=n)   # permuted, flipped, duplicated, with self-loops
    _same(g.louvain_levels(), want)
    g.set_memory_budget(1)
    _same(g.louvain_levels(), want)
    g.set_memory_budget(0)
    _same(g.louvain_levels(), want)   # a further call on the same handle
    g.close()


def test_seed_and_caps():
    n, e = _graphs()["gnp3000"]
    g = gr.CentralityGraph(e, n=n)
    _same(g.louvain_levels(seed=1), _want("gnp3000", seed=1))
    assert not np.array_equal(_want("gnp3000", seed=1)[0][-1], _want("gnp3000")[0][-1])
    _same(g.louvain_levels(seed=2 ** 64 - 3, max_levels=2, max_rounds=7), ref.louvain(n, e, 2 ** 64 - 3, 2, 7))
    g.close()


@pytest.mark.parametrize("name", ["gnp3000", "ladder", "two_triangles", "no_edges"])
def test_modularity_terms_on_random_labellings(name):
    n, e = _graphs()[name]
    g = gr.CentralityGraph(ref.messy(n, e, seed=1), n=n)
    rng = np.random.default_rng(4)
    labellings = [np.arange(n)[::-1].copy(), np.full(n, n - 1), _want(name)[0][-1]]
    labellings += [rng.integers(0, min(hi, n), size=n) for hi in (2, 50, n)]
    for labels in labellings:
        assert g.modularity_terms(labels) == ref.modularity_terms(n, e, labels)
    with pytest.raises(ValueError):
        g.modularity_terms(np.full(n, n))
    g.close()


def test_native_argument_checks():
    h = _native.CentGraph(3, [[0, 1]])
    with pytest.raises(ValueError, match=r"label of vertex 1 outside \[0, n\)"):
        h.modularity([0, 3, 0])
    with pytest.raises(ValueError, match="must be >= 1"):
        h.louvain(max_rounds=0)
    h.close()
    with pytest.raises(ValueError, match="handle is NULL"):
        h.modularity([0, 0, 0])
    with pytest.raises(ValueError, match="handle is NULL"):
        h.louvain()


class _ReferenceHandle:
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


def test_public_functions_equal_the_same_functions_over_the_stand_in(monkeypatch):
    import networkx as nx
    n, e, planted = ref.planted()["relaxed"]
    G = nx.relabel_nodes(nx.from_edgelist(e.tolist()), {i: f"v{i}" for i in range(n)})
    assert G.number_of_nodes() == n

    def everything():
        parts = gr.louvain_partitions(G, seed=3)
        return (gr.louvain_communities(G, seed=3), parts, gr.community_labels(G, seed=3).tolist(),
                gr.community_labels(G, level=0).tolist(), [gr.modularity(G, p) for p in parts],
                gr.modularity(e, planted), gr.louvain_communities(e, max_level=1))

    on_device = everything()
    monkeypatch.setattr(_native, "CentGraph", _ReferenceHandle)
    assert on_device == everything()
    assert on_device[0] == on_device[1][-1] and sum(map(len, on_device[0])) == n
