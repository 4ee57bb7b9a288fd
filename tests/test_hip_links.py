"""gh_cent_link_scores / gh_cent_link_candidates (csrc/links.hip) and graphem-rapids_amd/links.py on the device: against the
restatement (tests/links_reference.py) array for array, against themselves (memory budget, slab reuse, other calls on the
handle in between, edge order, duplicates, self-loops), and the public layer against networkx.  Every device quantity is an
integer, so every comparison with the restatement is exact."""
import networkx as nx
import numpy as np
import pytest

import graphem_rapids_amd as gr
from graphem_rapids_amd import _native

import links_reference as ref

pytestmark = pytest.mark.gpu

KS = (1, 3, 128)


@pytest.fixture(scope="module")
def handles():
    """One handle per named graph, opened on first use and closed with the module."""
    opened = {}

    def get(name):
        if name not in opened:
            _, n, e = ref.graph(name)
            opened[name] = gr.CentralityGraph(e, n=n)
        return opened[name]
    yield get
    for g in opened.values():
        g.close()


def _same_pairs(g, n, e, pairs):
    got = g.link_scores(pairs)
    want = ref.pair_scores(n, e, pairs)
    for have, key in zip(got, ("cn", "aa", "ra")):
        assert have.dtype == np.int64 and have.shape == want[key].shape and np.array_equal(have, want[key]), key
    return got


def _same_candidates(got, want):
    for have, need, dtype in zip(got, want, (np.int32, np.int64, np.int64)):
        assert have.dtype == dtype and have.shape == need.shape and np.array_equal(have, need)


# ---- pair kernel -----------------------------------------------------------------------------------------------------
def test_pairs_over_every_row_length(handles):
    _, n, e = ref.graph("rows")
    g = handles("rows")
    assert sorted(set(g.degree().tolist())) == [0, 1, 2, 3, 4, 63, 64, 65, 300]
    pairs = ref.row_length_pairs()
    cn, aa, ra = _same_pairs(g, n, e, pairs)
    at = {tuple(p): i for i, p in enumerate(pairs.tolist())}
    assert cn[at[(ref.HUB, ref.HUB)]] == 300 and cn[at[(ref.A63, ref.C65)]] == 63 and cn[at[(ref.C65, ref.B64)]] == 64
    assert cn[at[(ref.LONE, ref.HUB)]] == 0 and cn[at[(ref.LONE, ref.LONE)]] == 0 and cn[at[(ref.HUB, 7)]] == 0
    assert cn[at[(5, 9)]] == 4 and cn[at[(200, 201)]] == 1
    assert ra[at[(200, 201)]] == ((1 << 33) + 300) // 600 and aa[at[(200, 201)]] == _native.link_weight("adamic_adar", 300)


@pytest.mark.parametrize("name", ["ba300", "caveman", "dense130", "n65", "star300", "k5"])
def test_pairs_at_every_group_width(handles, name):
    """Mean degrees 2 to 65: the group is 4, 8 and 64 lanes wide."""
    _, n, e = ref.graph(name)
    rng = np.random.default_rng(1)
    pairs = np.concatenate([rng.integers(0, n, size=(600, 2)), ref.canonical_edges(n, e)[:100], [[0, 0], [n - 1, n - 1]]])
    _same_pairs(handles(name), n, e, pairs)


def test_pairs_in_chunks_null_outputs_and_refusals(handles):
    _, n, e = ref.graph("ba300")
    g = handles("ba300")
    pairs = np.random.default_rng(2).integers(0, n, size=(1000, 2))
    whole = g.link_scores(pairs)
    g.set_memory_budget(32 * 7)   # seven pairs at once
    try:
        for a, b in zip(whole, g.link_scores(pairs)):
            assert np.array_equal(a, b)
    finally:
        g.set_memory_budget(0)
    for j in range(3):
        want = [i != j for i in range(3)]
        part = g._g.link_scores(pairs, *want)   # pylint: disable=protected-access
        assert part[j] is None and all(np.array_equal(part[i], whole[i]) for i in range(3) if i != j)
    for arr in g.link_scores(np.zeros((0, 2), dtype=np.int64)):
        assert arr.shape == (0,) and arr.dtype == np.int64
    lib, h = _native.load(), g._g.handle   # pylint: disable=protected-access
    out = np.full(2, -7, dtype=np.int64)
    bad = np.array([[0, 1], [3, n]], dtype=np.int32)
    assert lib.gh_cent_link_scores(h, 2, _native.ptr(bad), _native.ptr(out), None, None) == _native.GH_ERR_INVALID
    assert lib.gh_cent_last_error(h) == b"pair 1 has a vertex id outside [0, n)" and (out == -7).all()
    assert lib.gh_cent_link_scores(h, 0, None, None, None, None) == _native.GH_OK
    with pytest.raises(ValueError):
        g.link_scores([[0, -1]])


# ---- candidate kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", range(5))
@pytest.mark.parametrize("name", ref.CANDIDATE_GRAPHS)
def test_candidates_are_the_restatement(handles, name, kind):
    _, n, _ = ref.graph(name)
    g = handles(name)
    ranked = ref.ranked_of(name, kind)
    rows = np.arange(n) if n <= 300 else np.array([300, 1, 64, 65, ref.A63, ref.C65, ref.LONE, ref.HUB, 299])
    if name == "star300":
        rows = np.array([5, 300, 0, 5])   # leaves: 299 candidates, all tied; the centre: none
    for k in KS:
        _same_candidates(g.link_candidates(kind, k, rows), ref.candidates(ranked, k, rows.tolist()))
    shuffled = np.random.default_rng(kind).permutation(np.concatenate([rows, rows[: 1 + len(rows) // 2]]))
    _same_candidates(g.link_candidates(ref.KINDS[kind], 3, shuffled), ref.candidates(ranked, 3, shuffled.tolist()))


def test_candidate_cases_say_what_they_should(handles):
    ids, num, den = handles("k5").link_candidates(ref.AA, 3, None)
    assert (ids == -1).all() and (num == 0).all() and (den == 1).all() and ids.shape == (5, 3)
    ids, _, _ = handles("triangle_tail").link_candidates(ref.CN, 3, [0, 4])
    assert ids.tolist() == [[3, -1, -1], [2, -1, -1]]   # from 0: not 1 (adjacent, and two hops away through 2), not 0
    ids, num, den = handles("c7").link_candidates(ref.JACCARD, 3, [0, 3])
    assert ids.tolist() == [[2, 5, -1], [1, 5, -1]] and num[0].tolist() == [1, 1, 0] and den[0].tolist() == [3, 3, 1]
    ids, _, _ = handles("k34").link_candidates(ref.RA, 128, [0, 3])
    assert ids[0, :3].tolist() == [1, 2, -1] and ids[1, :4].tolist() == [4, 5, 6, -1]
    ids, num, _ = handles("star300").link_candidates(ref.PA, 128, [7])
    assert ids[0].tolist() == [v for v in range(1, 130) if v != 7] and (num == 1).all()
    ids, _, _ = handles("isolated_source").link_candidates(ref.CN, 3, [6, 0])
    assert ids.tolist() == [[-1, -1, -1], [2, 4, -1]]
    sizes = [len(c) for name in ("ba300", "caveman") for c in ref.ranked_of(name, ref.CN)]
    assert min(sizes) < 128 < max(sizes)   # k below, at (1 and 3 occur in the small graphs) and above the list's length


def test_candidate_refusals(handles):
    g = handles("c7")
    lib, h = _native.load(), g._g.handle   # pylint: disable=protected-access
    ids, num = np.full(4, -7, dtype=np.int32), np.full(4, -7, dtype=np.int64)
    rows = np.array([0, 7], dtype=np.int32)
    call = lambda kind, k, count: lib.gh_cent_link_candidates(h, kind, k, count, _native.ptr(rows), _native.ptr(ids),   # noqa: E731
                                                              _native.ptr(num), _native.ptr(num))
    assert call(0, 2, 2) == _native.GH_ERR_INVALID and lib.gh_cent_last_error(h) == b"row 1 has a vertex id outside [0, n)"
    assert call(0, 0, 1) == _native.GH_ERR_INVALID and call(0, 129, 1) == _native.GH_ERR_INVALID
    assert lib.gh_cent_last_error(h) == b"k must lie in [1, 128]"
    assert call(5, 2, 1) == _native.GH_ERR_INVALID and call(-1, 2, 1) == _native.GH_ERR_INVALID
    assert call(0, 2, 0) == _native.GH_OK and (ids == -7).all() and (num == -7).all()
    for k in (0, 129):
        with pytest.raises(ValueError):
            g.link_candidates(0, k, [0])
    with pytest.raises(ValueError):
        g.link_candidates(0, 2, [7])


# ---- a pure function of the edge set and the arguments ---------------------------------------------------------------
@pytest.mark.parametrize("kind", [ref.JACCARD, ref.AA])
def test_budget_slab_reuse_and_other_calls_in_between(handles, kind):
    _, n, _ = ref.graph("ba300")
    g = handles("ba300")
    rows = np.arange(n)
    want = ref.candidates(ref.ranked_of("ba300", kind), 128, rows.tolist())
    g.set_memory_budget(20 * n)   # exactly one slab: 300 sources pass through it, each must find it clean
    try:
        _same_candidates(g.link_candidates(kind, 128, rows), want)
        g.set_memory_budget(2 * 20 * n + 19)   # two
        _same_candidates(g.link_candidates(kind, 128, rows), want)
    finally:
        g.set_memory_budget(0)
    _same_candidates(g.link_candidates(kind, 128, rows), want)
    g.core_layers()
    g.triangle_counts()
    _same_candidates(g.link_candidates(kind, 128, rows), want)


@pytest.mark.parametrize("name", ["caveman", "rows"])
def test_messy_edge_lists_give_the_same_arrays(handles, name):
    _, n, e = ref.graph(name)
    clean = handles(name)
    rows = np.arange(n)[:: max(1, n // 80)]
    pairs = np.random.default_rng(5).integers(0, n, size=(400, 2))
    g = gr.CentralityGraph(ref.messy(n, e, seed=9), n=n)
    try:
        assert np.array_equal(g.edges, clean.edges)
        for a, b in zip(g.link_scores(pairs), clean.link_scores(pairs)):
            assert np.array_equal(a, b)
        for kind in range(5):
            _same_candidates(g.link_candidates(kind, 3, rows), clean.link_candidates(kind, 3, rows))
    finally:
        g.close()


# ---- the public layer ------------------------------------------------------------------------------------------------
def test_networkx_names_on_the_device():
    G = ref.graph("caveman")[0]
    ebunch = [tuple(p) for p in np.random.default_rng(4).integers(0, 72, size=(300, 2)).tolist() if p[0] != p[1]]
    cn = np.array([len(list(nx.common_neighbors(G, u, v))) for u, v in ebunch])
    for fn in ("jaccard_coefficient", "preferential_attachment"):
        assert getattr(gr, fn)(G, ebunch) == [(u, v, p) for u, v, p in getattr(nx, fn)(G, ebunch)]
    for fn in ("adamic_adar_index", "resource_allocation_index"):
        got, want = getattr(gr, fn)(G, ebunch), list(getattr(nx, fn)(G, ebunch))
        assert [t[:2] for t in got] == ebunch
        err = np.abs(np.array([p for _, _, p in got]) - np.array([p for _, _, p in want]))
        assert (err <= cn * 2.0 ** -32).all()
    theirs = {(min(u, v), max(u, v)): p for u, v, p in nx.adamic_adar_index(G)}
    ours = gr.adamic_adar_index(G)
    assert [t[:2] for t in ours] == sorted(theirs) and all(abs(p - theirs[(u, v)]) <= 11 * 2.0 ** -32 for u, v, p in ours)
    best = gr.top_links(G, 5, "resource_allocation")
    assert [t[:2] for t in best] == [t[:2] for t in sorted(gr.resource_allocation_index(G), key=lambda t: (-t[2], t[0], t[1]))[:5]]
    out = gr.link_candidates(G, k=4, score="jaccard", sources=[9, 2])
    _same_candidates((out["ids"], out["num"], out["den"]), ref.candidates(ref.ranked_of("caveman", ref.JACCARD), 4, [9, 2]))
    assert np.array_equal(out["scores"], out["num"] / out["den"])


def test_link_prediction_benchmark():
    res = gr.link_prediction_benchmark(gr.generate_sbm, dict(n_per_block=60, num_blocks=4, p_in=0.3, p_out=0.01),
                                       num_iterations=30)
    methods = ("embedding", "common_neighbors", "jaccard", "adamic_adar", "resource_allocation", "preferential_attachment")
    assert gr.links.LINK_METHODS == methods
    for name in methods:
        assert 0.0 <= res[name]["auc"] <= 1.0 and 0.0 <= res[name]["average_precision"] <= 1.0, name
    n, k = res["n"], res["n_test"]
    assert n == 240 and k == len(res["test_edges"]) == len(res["negative_pairs"]) == round(0.1 * res["m"])
    assert res["n_train"] == res["m"] - k and res["layout_time"] > 0 and res["score_time"] > 0
    T = nx.empty_graph(n)
    T.add_edges_from(res["train_edges"].tolist())
    ebunch = [tuple(p) for p in np.concatenate([res["test_edges"], res["negative_pairs"]]).tolist()]
    theirs = {"common_neighbors": [len(list(nx.common_neighbors(T, u, v))) for u, v in ebunch]}
    for key, fn in (("jaccard", nx.jaccard_coefficient), ("adamic_adar", nx.adamic_adar_index),
                    ("resource_allocation", nx.resource_allocation_index), ("preferential_attachment", nx.preferential_attachment)):
        theirs[key] = [float(p) for _, _, p in fn(T, ebunch)]
    for key, scores in theirs.items():
        assert res[key]["auc"] == pytest.approx(gr.ranking_auc(scores[:k], scores[k:]), abs=1e-12), key
