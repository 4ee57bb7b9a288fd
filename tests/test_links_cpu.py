"""Link scores without a GPU: the exported C ABI and gh_link_weight, the restatement (tests/links_reference.py) against
networkx on the graphs of tests/test_hip_links.py, top_links' host merge against a global sort, and the Python layer of
graphem-rapids_amd/links.py over a stand-in handle that answers from the restatement."""
import ctypes
import math
import os
from fractions import Fraction

import networkx as nx
import numpy as np
import pytest

import graphem_rapids_amd as gr
from graphem_rapids_amd import _native, links

import links_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LINK_SYMBOLS = ["gh_link_weight", "gh_cent_link_scores", "gh_cent_link_candidates"]
PUBLIC = ["link_scores", "jaccard_coefficient", "adamic_adar_index", "resource_allocation_index", "preferential_attachment",
          "link_candidates", "top_links", "split_edges", "embedding_link_scores", "ranking_auc", "average_precision",
          "link_prediction_benchmark"]


# ---- the ABI ---------------------------------------------------------------------------------------------------------
def test_link_symbols_declared_exported_and_listed():
    from graphem_rapids_amd import build as gra_build
    header = open(os.path.join(ROOT, "include", "graphem_hip.h")).read()
    assert header.index("---- edge-list ingestion") < header.index("---- link scores") < header.index("gh_device_count")
    gra_build.build()
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in LINK_SYMBOLS:
        assert name + "(" in header, name
        assert name in _native.SYMBOLS and name in _native.SIGNATURES, name
        assert hasattr(lib, name), name
    assert len(_native.SIGNATURES["gh_cent_link_scores"][1]) == 6 and len(_native.SIGNATURES["gh_cent_link_candidates"][1]) == 8
    for i, name in enumerate(["GH_LINK_CN", "GH_LINK_JACCARD", "GH_LINK_AA", "GH_LINK_RA", "GH_LINK_PA"]):
        assert f"{name} = {i}" in header
    assert list(_native.LINK_KINDS.values()) == list(range(5)) and list(_native.LINK_KINDS) == ref.KINDS


def test_null_handle_is_refused_without_a_device():
    lib = _native.load()
    out = np.zeros(4, dtype=np.int64)
    ids = np.zeros(4, dtype=np.int32)
    assert lib.gh_cent_link_scores(None, 1, _native.ptr(ids), _native.ptr(out), None, None) == _native.GH_ERR_INVALID
    assert lib.gh_cent_last_error(None) == b"handle is NULL"
    assert lib.gh_cent_link_candidates(None, 0, 2, 1, _native.ptr(ids), _native.ptr(ids), _native.ptr(out),
                                       _native.ptr(out)) == _native.GH_ERR_INVALID
    assert lib.gh_cent_last_error(None) == b"handle is NULL"


def test_public_names_are_exported():
    for name in PUBLIC:
        assert name in gr.__all__, name
        assert getattr(gr, name) is getattr(links, name)
    assert "links" in gr.__all__ and gr.links is links
    for name in ("link_scores", "link_candidates"):
        assert callable(getattr(gr.CentralityGraph, name)) and callable(getattr(_native.CentGraph, name))
    assert links.MAX_ALL_PAIRS_VERTICES == 4096 and links.LINK_SCORES == tuple(ref.KINDS)


# ---- the weights -----------------------------------------------------------------------------------------------------
def test_resource_allocation_weight_is_the_integer_formula():
    lib = _native.load()
    assert lib.gh_link_weight(ref.RA, 0) == 0
    for d in range(1, 100001):
        assert lib.gh_link_weight(ref.RA, d) == ((1 << 33) + d) // (2 * d), d
    # 2^32 / d rounded half up
    assert lib.gh_link_weight(ref.RA, 1) == 1 << 32 and lib.gh_link_weight(ref.RA, 3) == 1431655765
    assert lib.gh_link_weight(ref.RA, 1 << 13) == 1 << 19


def test_adamic_adar_weight_is_within_half_a_unit():
    lib = _native.load()
    assert lib.gh_link_weight(ref.AA, 0) == 0 and lib.gh_link_weight(ref.AA, 1) == 0
    worst = 0.0
    for d in range(2, 100001):
        w = lib.gh_link_weight(ref.AA, d)
        worst = max(worst, abs(w - 4294967296.0 / math.log(d)))
    assert worst <= 0.5 + 2.0 ** -20
    assert lib.gh_link_weight(ref.AA, 2) == round(Fraction(2 ** 32) / Fraction(math.log(2)))


def test_weight_of_the_counting_kinds_and_refusals():
    lib = _native.load()
    for kind in (ref.CN, ref.JACCARD, ref.PA):
        assert lib.gh_link_weight(kind, 0) == lib.gh_link_weight(kind, 77) == 1
    assert lib.gh_link_weight(5, 3) == -1 and lib.gh_link_weight(-1, 3) == -1
    assert lib.gh_link_weight(ref.RA, -1) == -1 and lib.gh_link_weight(ref.AA, 1 << 30) == -1
    assert lib.gh_link_weight(ref.AA, (1 << 30) - 1) > 0
    assert _native.link_weight("adamic_adar", 7) == lib.gh_link_weight(ref.AA, 7)
    with pytest.raises(ValueError):
        _native.link_weight("adamic_adar", -3)


# ---- the restatement equals networkx ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ref.NETWORKX_GRAPHS)
def test_restatement_is_networkx(name):
    G, n, e = ref.graph(name)
    pairs = ref.all_pairs(n)
    ebunch = [tuple(p) for p in pairs.tolist()]
    got = ref.pair_scores(n, e, pairs)
    cn = np.array([len(list(nx.common_neighbors(G, u, v))) for u, v in ebunch])
    uni = np.array([len(set(G[u]) | set(G[v])) for u, v in ebunch])
    assert np.array_equal(got["cn"], cn) and np.array_equal(got["uni"], uni)
    assert got["pa"].tolist() == [p for _, _, p in nx.preferential_attachment(G, ebunch)]
    # a common neighbour of degree 1 occurs only at u = v: weight 0 here, a division by log 1 = 0 in networkx
    ok = np.array([all(G.degree(w) > 1 for w in nx.common_neighbors(G, u, v)) for u, v in ebunch])
    assert (pairs[~ok][:, 0] == pairs[~ok][:, 1]).all()
    want = np.array([p for _, _, p in nx.adamic_adar_index(G, [p for p, fine in zip(ebunch, ok) if fine])])
    err = np.abs(got["aa"][ok] / 2.0 ** 32 - want)
    assert (err <= cn[ok] * 2.0 ** -32).all(), float(err.max())
    want = np.array([p for _, _, p in nx.resource_allocation_index(G, ebunch)])
    err = np.abs(got["ra"] / 2.0 ** 32 - want)
    assert (err <= cn * 2.0 ** -32).all(), float(err.max())
    jac = np.divide(got["cn"], got["uni"], out=np.zeros(len(pairs)), where=got["uni"] > 0)
    want = np.array([float(p) for _, _, p in nx.jaccard_coefficient(G, ebunch)])
    assert jac.tobytes() == want.tobytes()


def test_candidates_of_the_restatement_are_the_vertices_at_distance_two():
    for name in ("ba300", "caveman", "triangle_tail", "isolated_source"):
        G, n, _ = ref.graph(name)
        ranked = ref.ranked_of(name, ref.CN)
        for u in range(n):
            at_two = {v for v, d in nx.single_source_shortest_path_length(G, u, cutoff=2).items() if d == 2}
            assert {v for v, _, _ in ranked[u]} == at_two
    sizes = {len(c) for c in ref.ranked_of("ba300", ref.CN)} | {len(c) for c in ref.ranked_of("caveman", ref.CN)}
    assert min(sizes) < 128 < max(sizes) and min(sizes) > 3


# ---- top_links' merge --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ba300", "caveman", "c7", "k34", "k5"])
@pytest.mark.parametrize("kind", range(5))
def test_top_links_merge_is_the_global_sort(name, kind):
    _, n, _ = ref.graph(name)
    ranked = ref.ranked_of(name, kind)
    everything = sorted(((u, v, a, b) for u in range(n) for v, a, b in ranked[u] if u < v),
                        key=lambda t: (-Fraction(t[2], t[3]), t[0], t[1]))
    for k in (1, 3, 10, 128):
        ids, num, den = ref.candidates(ranked, k, range(n))
        u, v, a, b = links._merge_top(np.arange(n), ids, num, den, k)   # pylint: disable=protected-access
        assert list(zip(u.tolist(), v.tolist(), a.tolist(), b.tolist())) == everything[:k], k


# ---- the Python layer over a stand-in handle -------------------------------------------------------------------------
class _ReferenceHandle:
    """What _native.CentGraph offers links.py, answered by the restatement."""
    built = 0

    def __init__(self, n, edges, device_id=0):
        del device_id
        type(self).built += 1
        self.n, self.e = int(n), np.asarray(edges, dtype=np.int64).reshape(-1, 2)

    def link_scores(self, pairs):
        s = ref.pair_scores(self.n, self.e, pairs)
        return s["cn"], s["aa"], s["ra"]

    def link_candidates(self, kind, k, rows):
        kind = _native.LINK_KINDS[kind] if isinstance(kind, str) else kind
        if not 1 <= int(k) <= 128:
            raise ValueError("k must lie in [1, 128]")
        return ref.candidates(ref.ranked_candidates(self.n, self.e, kind), int(k), np.asarray(rows).tolist())

    def close(self):
        pass


@pytest.fixture
def host_only(monkeypatch):
    monkeypatch.setattr(_native, "CentGraph", _ReferenceHandle)
    _ReferenceHandle.built = 0


NX_NAMES = [("jaccard_coefficient", "jaccard"), ("adamic_adar_index", "adamic_adar"),
            ("resource_allocation_index", "resource_allocation"), ("preferential_attachment", "preferential_attachment")]


def test_networkx_names_on_a_labelled_graph(host_only):
    B = ref.graph("caveman")[0]
    names = {i: f"v{(7 * i) % 72}" for i in range(72)}   # not in sorted order
    G = nx.relabel_nodes(B, names)
    nodes = list(G.nodes())
    rng = np.random.default_rng(3)
    ebunch = [(nodes[a], nodes[b]) for a, b in rng.integers(0, 72, size=(200, 2)).tolist() if a != b]
    for fn, key in NX_NAMES:
        got = getattr(gr, fn)(G, ebunch)
        want = list(getattr(nx, fn)(G, ebunch))
        assert [(u, v) for u, v, _ in got] == ebunch == [(u, v) for u, v, _ in want]
        cn = [len(list(nx.common_neighbors(G, u, v))) for u, v in ebunch]
        for (_, _, p), (_, _, q), c in zip(got, want, cn):
            if key in ("jaccard", "preferential_attachment"):
                assert p == q and isinstance(p, int) == (key == "preferential_attachment")
            else:
                assert abs(p - q) <= c * 2.0 ** -32
    scores = gr.link_scores(G, ebunch)
    assert set(scores) == {"common_neighbors", "union", "jaccard", "adamic_adar", "resource_allocation", "preferential_attachment"}
    assert scores["common_neighbors"].dtype == scores["union"].dtype == scores["preferential_attachment"].dtype == np.int64
    assert scores["jaccard"].dtype == scores["adamic_adar"].dtype == np.float64
    assert scores["jaccard"].tolist() == [p for _, _, p in gr.jaccard_coefficient(G, ebunch)]
    with pytest.raises(nx.NodeNotFound):
        gr.jaccard_coefficient(G, [(nodes[0], "nobody")])
    with pytest.raises(nx.NodeNotFound):
        gr.adamic_adar_index(B, [(0, 72)])


def test_ebunch_none_is_every_non_edge_in_order_and_capped(host_only):
    G = ref.graph("n65")[0]
    want = sorted((min(u, v), max(u, v)) for u, v in nx.non_edges(G))
    for fn, _ in NX_NAMES:
        got = getattr(gr, fn)(G)
        assert [(u, v) for u, v, _ in got] == want
        theirs = {(min(u, v), max(u, v)): p for u, v, p in getattr(nx, fn)(G)}
        assert all(abs(p - theirs[(u, v)]) <= 11 * 2.0 ** -32 for u, v, p in got)
    e = ref.edge_array(G)
    assert gr.preferential_attachment(e) == gr.preferential_attachment(G) == gr.preferential_attachment(gr.edges_to_adjacency(65, e))
    big = np.array([[0, links.MAX_ALL_PAIRS_VERTICES]])
    with pytest.raises(ValueError, match="link_candidates"):
        gr.jaccard_coefficient(big)
    assert gr.jaccard_coefficient(big, [(0, 5)]) == [(0, 5, 0.0)]   # empty union: 0, as in networkx


def test_link_candidates_and_top_links(host_only):
    G, n, e = ref.graph("caveman")
    for score in ref.KINDS:
        kind = ref.KINDS.index(score)
        out = gr.link_candidates(G, k=5, score=score, sources=[7, 3, 7])
        ids, num, den = ref.candidates(ref.ranked_of("caveman", kind), 5, [7, 3, 7])
        assert out["sources"].tolist() == [7, 3, 7]
        assert np.array_equal(out["ids"], ids) and np.array_equal(out["num"], num) and np.array_equal(out["den"], den)
        scale = 2.0 ** 32 if score in ("adamic_adar", "resource_allocation") else 1.0
        assert out["scores"].dtype == np.float64 and np.array_equal(out["scores"], num / den / scale)
        top = gr.top_links(G, 10, score)
        assert len(top) == 10 and all(u < v and not G.has_edge(u, v) for u, v, _ in top)
        assert [p for _, _, p in top] == sorted((p for _, _, p in top), reverse=True)
    everyone = gr.link_candidates(e, k=3)
    assert everyone["sources"].tolist() == list(range(n)) and everyone["ids"].shape == (n, 3)
    best = gr.top_links(G, 1, "adamic_adar")[0]
    theirs = max(nx.adamic_adar_index(G), key=lambda t: t[2])
    assert abs(best[2] - theirs[2]) <= 11 * 2.0 ** -32
    with pytest.raises(ValueError):
        gr.link_candidates(G, score="katz")
    with pytest.raises(ValueError):
        gr.top_links(G, 129)
    assert gr.top_links(nx.complete_graph(5), 4) == []


# ---- splits and rankings: host code, no handle ------------------------------------------------------------------------
@pytest.mark.parametrize("name,fraction", [("ba300", 0.1), ("caveman", 0.25), ("n65", 0.1)])
def test_split_edges(name, fraction):
    G, n, e = ref.graph(name)
    split = gr.split_edges(G, test_fraction=fraction, seed=4)
    train, test, neg = split["train_edges"], split["test_edges"], split["negative_pairs"]
    full = {tuple(p) for p in ref.canonical_edges(n, e).tolist()}
    assert split["n"] == n and len(test) == round(fraction * len(full)) == len(neg)
    tr, te = {tuple(p) for p in train.tolist()}, {tuple(p) for p in test.tolist()}
    assert not tr & te and tr | te == full and len(tr) == len(train) and len(te) == len(test)
    H = nx.empty_graph(n)
    H.add_edges_from(train.tolist())
    assert nx.number_connected_components(H) == nx.number_connected_components(G)
    ng = {tuple(p) for p in neg.tolist()}
    assert len(ng) == len(neg) and not ng & full and all(a < b for a, b in ng)
    again = gr.split_edges(e, test_fraction=fraction, seed=4)
    assert all(np.array_equal(split[key], again[key]) for key in ("train_edges", "test_edges", "negative_pairs"))
    other = gr.split_edges(G, test_fraction=fraction, seed=5)
    assert not np.array_equal(other["test_edges"], test)


def test_split_edges_refusals():
    tree = nx.balanced_tree(2, 4)
    with pytest.raises(ValueError, match="spanning forest"):
        gr.split_edges(tree, 0.2)
    loose = gr.split_edges(tree, 0.2, keep_connected=False)
    assert len(loose["test_edges"]) == 6
    with pytest.raises(ValueError, match="non-edges"):
        gr.split_edges(nx.complete_graph(6), 0.2, keep_connected=False)
    for bad in (0.0, 1.0, -0.1):
        with pytest.raises(ValueError):
            gr.split_edges(tree, bad)
    with pytest.raises(ValueError):
        gr.split_edges(nx.path_graph(3), 0.1, keep_connected=False)   # rounds to no test edge
    with pytest.raises(NotImplementedError):
        gr.split_edges(nx.DiGraph([(0, 1), (1, 2)]), 0.5)


def _brute_auc(pos, neg):
    total = 0.0
    for p in pos:
        for q in neg:
            total += 1.0 if p > q else 0.5 if p == q else 0.0
    return total / (len(pos) * len(neg))


def _brute_average_precision(pos, neg):
    """Walk the distinct scores from the top; at each, everything scored at least that much is retrieved."""
    total, before = 0.0, 0
    for t in sorted(set(pos) | set(neg), reverse=True):
        tp = sum(1 for p in pos if p >= t)
        fp = sum(1 for q in neg if q >= t)
        total += (tp - before) / len(pos) * (tp / (tp + fp))
        before = tp
    return total


def test_ranking_auc_and_average_precision_against_double_loops():
    rng = np.random.default_rng(8)
    cases = [(rng.integers(0, 6, 40), rng.integers(0, 5, 55)),       # many ties
             (rng.standard_normal(30) + 1, rng.standard_normal(70)),  # none
             (np.array([2.0, 2.0]), np.array([2.0, 2.0, 2.0])),       # nothing but ties
             (np.array([3.0]), np.array([1.0, 2.0])), (np.array([0.0]), np.array([1.0]))]
    for pos, neg in cases:
        assert gr.ranking_auc(pos, neg) == pytest.approx(_brute_auc(pos.tolist(), neg.tolist()), abs=1e-15)
        assert gr.average_precision(pos, neg) == pytest.approx(_brute_average_precision(pos.tolist(), neg.tolist()), abs=1e-12)
    assert gr.ranking_auc([2.0, 2.0], [2.0, 2.0, 2.0]) == 0.5 and gr.ranking_auc([3.0], [1.0, 2.0]) == 1.0
    assert gr.average_precision([3.0], [1.0, 2.0]) == 1.0 and gr.average_precision([0.0], [1.0]) == 0.5
    assert math.isnan(gr.ranking_auc([], [1.0])) and math.isnan(gr.average_precision([], [1.0]))


def test_embedding_link_scores():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((20, 3))
    pairs = rng.integers(0, 20, size=(50, 2))
    got = gr.embedding_link_scores(x, pairs)
    x32 = x.astype(np.float32).astype(np.float64)
    want = [-float(((x32[a] - x32[b]) ** 2).sum()) for a, b in pairs.tolist()]
    assert got.dtype == np.float64 and np.allclose(got, want, rtol=1e-15, atol=0)

    class Embedder:
        positions = x.astype(np.float32)

        def run_layout(self):
            pass
    assert np.array_equal(gr.embedding_link_scores(Embedder(), pairs), got)
    with pytest.raises(ValueError):
        gr.embedding_link_scores(x, [[0, 20]])


def test_heuristic_aucs_of_a_split_are_networkx(host_only):
    """What link_prediction_benchmark does after the layout, on the host: the five predictors on the train graph of a split,
    read by ranking_auc, against networkx's scores on the same split."""
    _, n, e = ref.graph("ba300")
    split = gr.split_edges(e, 0.1, seed=0)
    pairs = np.concatenate([split["test_edges"], split["negative_pairs"]])
    T = nx.empty_graph(n)
    T.add_edges_from(split["train_edges"].tolist())
    g = gr.CentralityGraph(split["train_edges"], n=n)
    ours = links._scores(g, pairs)   # pylint: disable=protected-access
    k = len(split["test_edges"])
    ebunch = [tuple(p) for p in pairs.tolist()]
    for fn, key in NX_NAMES:
        theirs = np.array([float(p) for _, _, p in getattr(nx, fn)(T, ebunch)])
        assert gr.ranking_auc(ours[key][:k], ours[key][k:]) == pytest.approx(gr.ranking_auc(theirs[:k], theirs[k:]), abs=1e-12)
