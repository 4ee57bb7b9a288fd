"""gh_ic_set_arc_probabilities, gh_ic_spread_arcs and gh_ic_rr_sample_arcs against the numpy restatement of the per-arc coin
rule (tests/arc_ic_reference.py), bit for bit per trial and id for id per RR set; the p forms of influence.py on top."""
import functools

import networkx as nx
import numpy as np
import pytest
import scipy.sparse as sp

import graphem_rapids_amd as gr
from graphem_rapids_amd import _native
from graphem_rapids_amd.influence import InfluenceGraph

import arc_ic_reference as arc
import ic_reference as ref
import ris_reference as ris

pytestmark = pytest.mark.gpu

SEED = 7
EXTRA = 3   # isolated vertices n .. n + 2 behind every graph, as tests/test_hip_influence.py adds them


_mixed = arc.mixed_probabilities   # exact 0, exact 1, 1e-9 and 1 - 1e-9 mixed in; tests/test_hip_cascade_caps.py shares it


@functools.lru_cache(maxsize=None)
def _graph(name):
    """(n without the isolated extras, canonical pairs, directed, prob in arc_probabilities' shape)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "star":        # hub row of 131 arcs: two full batches of 64 slots and a ragged third
        n, directed = 132, False
        pairs = np.column_stack([np.zeros(n - 1, dtype=np.int64), np.arange(1, n)])
        prob = np.column_stack([_mixed(rng, n - 1), _mixed(rng, n - 1)])   # hub -> leaf, leaf -> hub
    elif name == "undirected":
        n, directed = 400, False
        pairs = ref.canonical_arcs(n, rng.integers(0, n, (1640, 2)), False)
        prob = _mixed(rng, (len(pairs), 2), 0.15)
    elif name == "directed":
        n, directed = 400, True
        pairs = ref.canonical_arcs(n, rng.integers(0, n, (1700, 2)), True)
        pairs = pairs[np.sort(rng.choice(len(pairs), 1600, replace=False))]
        prob = _mixed(rng, len(pairs), 0.4)
    else:                     # path: a -> b live on the odd edges only, b -> a on the even ones
        n, directed = 50, False
        pairs = np.column_stack([np.arange(n - 1), np.arange(1, n)])
        prob = np.column_stack([np.arange(n - 1) % 2, 1 - np.arange(n - 1) % 2]).astype(np.float64)
    assert np.array_equal(pairs, ref.canonical_arcs(n, pairs, directed))
    return n, pairs, directed, prob


def _native_graph(name, budget=None):
    n, pairs, directed, prob = _graph(name)
    g = _native.ICGraph(n + EXTRA, pairs, directed)
    g.set_arc_probabilities(*arc.as_directed(pairs, directed, prob))
    if budget is not None:
        g.set_memory_budget(budget)
    return g


@functools.lru_cache(maxsize=None)
def _want(name, seeds, T, hops):
    n, pairs, directed, prob = _graph(name)
    return arc.spread_trials_arcs(n + EXTRA, pairs, directed, prob, list(seeds), T, SEED, hops)


def _seed_sets(name):
    """(sets of one batched call, the set that is evaluated alone).  Alone, the n / 16 + 5 seeds reach the pull threshold
    (sets in the call) * n / 16 in round 1; a single vertex goes through push."""
    n = _graph(name)[0] + EXTRA
    first = {"star": [0], "path": [25]}.get(name, [1])    # the star's hub; its leaves are in the other sets
    batched = [first, [], [1, 1, 5, 2, 5], [n - 1, n - 2, 2], [7]]
    alone = list(range(1, n, max(1, (n - 1) // (n // 16 + 5))))[:n // 16 + 5]
    assert len(set(alone)) == n // 16 + 5 >= max(1, n // 16) and 0 not in alone
    return batched, alone


@pytest.mark.parametrize("hops", [None, 0, 1, 3])
@pytest.mark.parametrize("T", [1, 64, 130])
@pytest.mark.parametrize("name", ["star", "undirected", "directed", "path"])
def test_per_trial_counts_identical(name, T, hops):
    batched, alone = _seed_sets(name)
    g = _native_graph(name)
    h = -1 if hops is None else hops
    tot, got = g.spread(batched, None, T, SEED, h, per_trial=True)
    tot1, got1 = g.spread([alone], None, T, SEED, h, per_trial=True)
    g.close()
    assert got.dtype == np.int32 and got.shape == (len(batched), T)
    assert np.array_equal(tot, got.sum(axis=1, dtype=np.int64)) and tot1[0] == got1.sum(dtype=np.int64)
    for s, row in zip(batched + [alone], list(got) + [got1[0]]):
        assert np.array_equal(row, _want(name, tuple(s), T, hops)), (name, s)


def test_equal_table_is_the_float_path_and_leaves_it_alone():
    n, pairs, directed, _ = _graph("undirected")
    sets = [[1], [3, 50, 50], list(range(0, n, 11))]
    g = InfluenceGraph(pairs, n=n + EXTRA)
    before = [g.spread(s, 0.3, 130, 3, SEED, return_trials=True)[1] for s in sets]
    table = [g.spread(s, np.full(len(pairs), 0.3), 130, 3, SEED, return_trials=True)[1] for s in sets]
    after = [g.spread(s, 0.3, 130, 3, SEED, return_trials=True)[1] for s in sets]
    other = g.spread(sets[2], 0.05, 130, None, SEED, return_trials=True)[1]   # a float call after a table was set
    g.close()
    for s, a, b, c in zip(sets, before, table, after):
        assert np.array_equal(a, ref.spread_trials(n + EXTRA, pairs, False, s, 0.3, 130, SEED, 3))
        assert np.array_equal(a, b) and np.array_equal(a, c)
    assert np.array_equal(other, ref.spread_trials(n + EXTRA, pairs, False, sets[2], 0.05, 130, SEED, None))


@pytest.mark.parametrize("name", ["undirected", "directed"])
def test_invariance_arc_order_duplicates_loops_batching_budget(name):
    n, pairs, directed, prob = _graph(name)
    rng = np.random.default_rng(0)
    sets = [[i, (7 * i) % n] for i in range(20)]
    a = _native_graph(name)
    _, t0 = a.spread(sets, None, 130, 11, -1, per_trial=True)
    a.close()
    # the same graph from shuffled arcs with duplicates and self-loops (undirected: edges written backwards as well),
    # the same table from a sparse matrix; the handle then lists the pairs in the canonical order again
    messy = pairs[rng.permutation(len(pairs))]
    if not directed:
        messy[::2] = messy[::2, ::-1]
    messy = np.concatenate([messy, messy[:100], np.column_stack([np.arange(50), np.arange(50)])])
    dp, dq = arc.as_directed(pairs, directed, prob)
    keep = dq != 0   # stored zeros would be fine; absent entries mean 0 too
    P = sp.csr_matrix((dq[keep], (dp[keep, 0], dp[keep, 1])), shape=(n + EXTRA, n + EXTRA))
    b = InfluenceGraph(messy, n=n + EXTRA, directed=directed)
    assert np.array_equal(b.arcs, pairs) and np.array_equal(b.arc_probabilities(P), prob)
    hops = b._hops(None)
    assert b._native_p(b._resolve(P)) is None
    assert np.array_equal(t0, b._ic.spread(sets, None, 130, 11, hops, per_trial=True)[1])
    parts = [b._ic.spread(sets[i:i + 7], None, 130, 11, hops, per_trial=True)[1] for i in range(0, len(sets), 7)]
    assert np.array_equal(t0, np.concatenate(parts))
    b._ic.set_memory_budget(1)   # one set per chunk
    assert np.array_equal(t0, b._ic.spread(sets, None, 130, 11, hops, per_trial=True)[1])
    # the pairs of the table in another order give the same table
    order = rng.permutation(len(dp))
    b._ic.set_arc_probabilities(dp[order], dq[order])
    assert np.array_equal(t0, b._ic.spread(sets, None, 130, 11, hops, per_trial=True)[1])
    b.close()


@pytest.mark.parametrize("hops", [None, 2])
def test_marginal_mode(hops):
    g = _native_graph("undirected")
    h = -1 if hops is None else hops
    base = [3, 10, 10, 77]
    cands = [[1], [3], [200], [], [5, 6]]
    _, marg = g.spread(cands, None, 130, 5, h, base=base, per_trial=True)
    _, full = g.spread([base + c for c in cands], None, 130, 5, h, per_trial=True)
    _, alone = g.spread([base], None, 130, 5, h, per_trial=True)
    g.close()
    assert np.array_equal(marg, full - alone) and full.any()


def _same(coll, want):
    indptr, members, roots = want
    assert coll.n_sets == len(roots) and coll.n_members == len(members)
    assert np.array_equal(coll.roots, roots)
    assert np.array_equal(coll.indptr, indptr)
    assert np.array_equal(coll.members, members)


@pytest.mark.parametrize("hops", [None, 2])
@pytest.mark.parametrize("name", ["undirected", "directed"])
def test_rr_sets_equal_the_restatement(name, hops):
    n, pairs, directed, prob = _graph(name)
    g = InfluenceGraph(pairs, n=n + EXTRA, directed=directed)
    coll = g.rr_sets(1100, prob, hops, SEED)     # default trials and roots; two chunks of the level machinery
    _same(coll, arc.rr_sets_arcs(n + EXTRA, pairs, directed, prob, 1100, SEED, hops))
    coll.extend(70)                              # the collection's own table, trials 1100 ..
    _same(coll, arc.rr_sets_arcs(n + EXTRA, pairs, directed, prob, 1170, SEED, hops))
    coll.close()
    rng = np.random.default_rng(3)
    trials = rng.integers(0, 2 ** 40, 130).astype(np.uint64)
    trials[5:9] = trials[4]
    roots = rng.integers(0, n + EXTRA, 130)
    roots[6] = roots[5]
    coll = g.rr_sets(130, prob, hops, SEED, trials=trials, roots=roots)
    _same(coll, arc.rr_sets_arcs(n + EXTRA, pairs, directed, prob, seed=SEED, max_hops=hops, trials=trials, roots=roots))
    coll.close()
    g.close()


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("hops", [None, 2])
def test_rr_identity_on_the_device(directed, hops):
    """n samples on trial t, one per root: count_hit(S) = the per-trial spread of S, both from the kernels."""
    n = 300
    rng = np.random.default_rng(8)
    pairs = ref.canonical_arcs(n, rng.integers(0, n, (1000, 2)), directed)
    prob = _mixed(rng, len(pairs) if directed else (len(pairs), 2), 0.5)
    g = InfluenceGraph(pairs, n=n, directed=directed)
    sets = [[0, 5, 5, 77], list(range(3, n, 41))]
    spread = [g.spread(s, prob, 65, hops, SEED, return_trials=True)[1] for s in sets]
    for t in (0, 64):
        coll = g.rr_sets(n, prob, hops, SEED, trials=np.full(n, t, dtype=np.uint64), roots=np.arange(n))
        for s, counts in zip(sets, spread):
            assert coll.count_hit(s) == counts[t]
        coll.close()
    g.close()


def _plain_greedy(n, pairs, directed, prob, k, T, hops, seed):
    cache = {}

    def f(s):
        key = tuple(sorted(set(s)))
        if key not in cache:
            cache[key] = int(arc.spread_trials_arcs(n, pairs, directed, prob, list(key), T, seed, hops).sum())
        return cache[key]
    seeds = []
    for _ in range(k):
        base = f(seeds)
        gains = [f(seeds + [v]) - base if v not in seeds else -1 for v in range(n)]
        seeds.append(int(np.argmax(gains)))
    return seeds


@pytest.mark.parametrize("directed", [False, True])
def test_greedy_weighted_cascade(directed):
    n = 60
    raw = np.random.default_rng(5).integers(0, n, (150, 2))
    g = InfluenceGraph(raw, n=n, directed=directed)
    uploads = []
    upload = g._ic.set_arc_probabilities
    g._ic.set_arc_probabilities = lambda pairs, prob: (uploads.append(len(prob)), upload(pairs, prob))
    lazy, evals = g.greedy(4, p="wc", n_trials=64, seed=9)
    plain, evals_plain = g.greedy(4, p="wc", n_trials=64, seed=9, celf=False)
    assert len(uploads) == 1   # one specification, one upload: every evaluation of both runs reused the table
    wc = g.arc_probabilities("wc")
    g.close()
    indeg = np.bincount(g.arcs[:, 1] if directed else g.arcs.ravel(), minlength=n)
    assert np.array_equal(wc if directed else wc[:, 0], 1.0 / indeg[g.arcs[:, 1]])
    assert lazy == plain == _plain_greedy(n, g.arcs, directed, wc, 4, 64, None, 9)
    assert evals <= evals_plain


def test_ris_weighted_cascade_is_max_coverage_of_the_restated_sets():
    n = 200
    raw = np.random.default_rng(6).integers(0, n, (700, 2))
    g = InfluenceGraph(raw, n=n)
    seeds, info = gr.ris_seed_selection(g, 5, p="wc", n_samples=2000, seed=4)
    wc = g.arc_probabilities("wc")
    # OPIM-C: both collections and every doubling find the one table in place
    uploads = []
    upload = g._ic.set_arc_probabilities
    g._ic.set_arc_probabilities = lambda pairs, prob: (uploads.append(len(prob)), upload(pairs, prob))
    opim, opim_info = gr.ris_seed_selection(g, 5, p="wc", epsilon=0.5, max_samples=600, seed=4)
    g.close()
    assert uploads == [] and len(set(opim)) == 5 and opim_info["samples"] <= 600
    indptr, members, _ = arc.rr_sets_arcs(n, g.arcs, False, wc, 2000, 4, 198)
    want, gains = ris.max_coverage(indptr, members, n, 5)
    assert seeds == want and info["covered"] == gains.sum() and info["samples"] == 2000


def test_public_entry_points_take_a_specification():
    G = nx.gnm_random_graph(80, 240, seed=2)
    value, iters = gr.ndlib_estimated_influence(G, [0, 7], p="wc", iterations_count=30, n_trials=64, seed=5)
    n, pairs, _, _ = gr.influence._graph_arcs(G)
    wc = gr.arc_probabilities(pairs, n, False, "wc")
    assert iters == 30 and value == arc.spread_trials_arcs(n, pairs, False, wc, [0, 7], 64, 5, 28).mean()
    tri = gr.trivalency_probabilities(pairs, False, seed=1, values=(0.5, 0.1, 0.01))
    mean, trials = gr.influence_spread(G, [0, 7], p=tri, n_trials=64, seed=5, return_trials=True)
    assert np.array_equal(trials, arc.spread_trials_arcs(n, pairs, False, tri, [0, 7], 64, 5, None)) and mean == trials.mean()
    seeds, total = gr.greedy_seed_selection(G, 2, p=sp.csr_matrix(nx.to_scipy_sparse_array(G) * 0.2), n_trials=32, seed=1)
    assert len(set(seeds)) == 2 and total > 0
    with pytest.raises(ValueError):
        gr.influence_spread(G, [0], p="lt")
    with pytest.raises(ValueError):
        gr.influence_spread(G, [0], p=np.full(len(pairs) + 1, 0.1))


def test_run_influence_benchmark_weighted_cascade():
    res = gr.run_influence_benchmark(gr.planted_partition_edges, {"n": 600, "communities": 4, "deg_in": 6, "deg_out": 1},
                                     k=5, p="wc", iterations=50, num_layout_iterations=5)
    keys = {"graph_type", "n", "m", "backend", "graphem_seeds", "greedy_seeds", "graphem_influence", "greedy_influence",
            "random_influence", "graphem_time", "greedy_time", "graphem_eval_time", "greedy_eval_time",
            "greedy_iterations", "graphem_norm_influence", "greedy_norm_influence", "random_norm_influence",
            "graphem_efficiency", "greedy_efficiency", "total_time"}
    assert keys <= set(res)
    assert res["n"] == 600 and len(res["greedy_seeds"]) == 5 and len(res["graphem_seeds"]) == 5
    assert 5 <= res["greedy_influence"] <= 600


def test_errors_and_a_failed_set_keeps_the_table():
    n, pairs, directed, prob = _graph("directed")
    g = _native.ICGraph(n + EXTRA, pairs, True)
    rr = _native.RRSets(n + EXTRA)
    with pytest.raises(ValueError, match="no arc probabilities"):
        g.spread([[0]], None, 8)
    with pytest.raises(ValueError, match="no arc probabilities"):
        g.rr_sample(rr, 4, None)
    assert rr.counts() == (0, 0)
    g.set_arc_probabilities(pairs, prob)
    _, t0 = g.spread([[1], [2, 3]], None, 70, SEED, per_trial=True)
    u, v = pairs[0]
    absent = next([a, b] for a in range(n) for b in range(n) if a != b and not ((pairs == [a, b]).all(axis=1)).any())
    bad = [([absent], [0.5], "not an arc"), ([[u, u]], [0.5], "not an arc"), ([[u, n + EXTRA]], [0.5], None),
           ([[u, v], [u, v]], [0.5, 0.5], "twice"), ([[u, v]], [np.nan], r"\[0, 1\]"), ([[u, v]], [1.5], r"\[0, 1\]"),
           ([[u, v]], [-0.25], r"\[0, 1\]"), ([[u, v]], [0.5, 0.5], None)]
    for bad_pairs, bad_prob, message in bad:
        with pytest.raises(ValueError, match=message):
            g.set_arc_probabilities(bad_pairs, bad_prob)
        assert np.array_equal(t0, g.spread([[1], [2, 3]], None, 70, SEED, per_trial=True)[1])   # the old table is in place
    # a call replaces the table; arcs that are not listed get threshold 0
    half = np.arange(len(pairs)) % 2 == 0
    g.set_arc_probabilities(pairs[half], prob[half])
    _, t1 = g.spread([[1], [2, 3]], None, 70, SEED, per_trial=True)
    for s, row in zip([[1], [2, 3]], t1):
        assert np.array_equal(row, arc.spread_trials_arcs(n + EXTRA, pairs, True, np.where(half, prob, 0.0), s, 70, SEED))
    for kw in (dict(n_trials=0), dict(max_hops=-2)):
        with pytest.raises(ValueError):
            g.spread([[0]], None, kw.get("n_trials", 8), 0, kw.get("max_hops", -1))
    with pytest.raises(ValueError):
        g.spread([[n + EXTRA]], None, 8)
    rr.close()
    g.close()
    # an undirected edge: each direction may be listed once, not twice
    e = _native.ICGraph(3, [[0, 1], [1, 2]])
    e.set_arc_probabilities([[0, 1], [1, 0], [2, 1]], [1.0, 0.0, 1.0])
    assert e.spread([[0], [1], [2]], None, 5).tolist() == [10, 5, 10]   # 0 -> 1 and 2 -> 1 are live, 1 -> 0 and 1 -> 2 are not
    with pytest.raises(ValueError, match="twice"):
        e.set_arc_probabilities([[1, 0], [1, 0]], [0.5, 0.5])
    e.close()
