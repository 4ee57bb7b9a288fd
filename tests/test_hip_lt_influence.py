"""gh_ic_set_lt_weights, gh_ic_spread_lt and gh_ic_rr_sample_lt against the numpy restatement of the Linear Threshold rule
(tests/lt_reference.py), bit for bit per trial and id for id per RR set; linear_threshold() through influence.py on top;
and the four Linear Threshold launches past IC_MAX_BLOCKS workgroups where the sizing rules let a shape get there
(tests/lt_caps.py)."""
import functools

import networkx as nx
import numpy as np
import pytest
import scipy.sparse as sp

import graphem_rapids_amd as gr
from graphem_rapids_amd import _native
from graphem_rapids_amd.influence import InfluenceGraph

import arc_ic_reference as arc
import cascade_caps as cc
import ic_reference as ref
import launch_caps as lc
import lt_caps
import lt_reference as lt
import ris_reference as ris

pytestmark = pytest.mark.gpu

SEED = 7
LT = _native.LT
GRAPHS = ["star65", "star130", "path", "gnp300", "out3"]


@functools.lru_cache(maxsize=None)
def _graph(name):
    """(n, canonical pairs, directed).  The stars are undirected: the hub's row has 65 / 130 arcs in both CSRs -- one and two
    batches of 64 slots and a tail -- and every leaf's row the one arc from the hub."""
    if name.startswith("star"):
        d = int(name[4:])
        return d + 1, np.column_stack([np.zeros(d, dtype=np.int64), np.arange(1, d + 1)]), False
    if name == "path":
        return 40, np.column_stack([np.arange(39), np.arange(1, 40)]), True
    if name == "gnp300":
        return 300, ref.canonical_arcs(300, gr.erdos_renyi_edges(300, 0.02, seed=4), False), False
    n = 300   # out-degree 3 on all but three isolated vertices
    return n, ref.canonical_arcs(n, cc._out_regular(n - 3, 3, np.random.default_rng(19)), True), True


@functools.lru_cache(maxsize=None)
def _weights(name, kind):
    n, pairs, directed = _graph(name)
    return gr.lt_weights(pairs, n, directed) if kind == "uniform" else lt.mixed_weights(sum(map(ord, name)), n, pairs, directed)


def _native_graph(name, kind, budget=None):
    n, pairs, directed = _graph(name)
    g = _native.ICGraph(n, pairs, directed)
    g.set_lt_weights(*arc.as_directed(pairs, directed, _weights(name, kind)))
    if budget is not None:
        g.set_memory_budget(budget)
    return g


@functools.lru_cache(maxsize=None)
def _want(name, kind, seeds, T, hops):
    """(per-trial counts, frontier entries per level) of one seed set evaluated alone."""
    n, pairs, directed = _graph(name)
    f = ref.Frontiers()
    return lt.spread_trials_lt(n, pairs, directed, _weights(name, kind), list(seeds), T, SEED, hops, frontiers=f), f.entries()


def _seed_sets(name):
    """(one vertex, n / 4 vertices): alone in a call, the first starts in push and the second in pull.  The first is
    vertex 0 -- the hub of a star, whose whole out-row round 1 pushes along; the second leaves it out, so that round 1
    pulls along the hub's in-row."""
    n = _graph(name)[0]
    return (0,), tuple(range(1, n, 4))[:n // 4]


@pytest.mark.parametrize("kind", ["uniform", "mixed"])
@pytest.mark.parametrize("name", GRAPHS)
def test_per_trial_counts_identical(name, kind):
    n = _graph(name)[0]
    pull_min = lc.ic_pull_min(lc.defines(), 1, n)
    g = _native_graph(name, kind)
    got = {(s, T, hops): g.spread([s], LT, T, SEED, -1 if hops is None else hops, per_trial=True)
           for s in _seed_sets(name) for T in (1, 64, 130) for hops in (None, 0, 1, 3)}
    g.close()
    sides = set()
    for (s, T, hops), (tot, trials) in got.items():
        want, entries = _want(name, kind, s, T, hops)
        assert trials.dtype == np.int32 and trials.shape == (1, T)
        assert np.array_equal(trials[0], want), (name, kind, s, T, hops)
        assert tot[0] == want.sum()
        if entries:   # round 1's frontier is the seed set: which launch did its work
            assert entries[0] == len(s)
            sides.add("pull" if entries[0] >= pull_min else "push")
            assert (len(s) == 1) == (entries[0] < pull_min)
    assert sides == {"push", "pull"}


def test_mixed_tables_hold_every_kind_of_row():
    """What the mixed tables above are meant to contain: rows that sum exactly to 1, rows well below, exact zeros, a single
    arc of weight 1, and a weight of 2^-33 whose interval is empty."""
    n, pairs, directed = _graph("out3")
    w = _weights("out3", "mixed")
    _, dst, lo, hi = lt.rows_of(n, pairs, directed, w)
    ws = w[np.lexsort((pairs[:, 0], pairs[:, 1]))]
    total = np.bincount(dst, weights=ws, minlength=n)
    assert (total == 1.0).any() and ((total > 0) & (total < 0.6)).any() and (ws == 0.0).any() and (ws == 1.0).any()
    assert ((ws == 2.0 ** -33) & (hi == lo)).any()


@pytest.mark.parametrize("name", ["gnp300", "out3"])
def test_invariance_arc_order_duplicates_loops_batching_budget(name):
    n, pairs, directed = _graph(name)
    weight = _weights(name, "mixed")
    rng = np.random.default_rng(0)
    sets = [[i, (7 * i) % n] for i in range(20)]
    a = _native_graph(name, "mixed")
    _, t0 = a.spread(sets, LT, 130, 11, -1, per_trial=True)
    a.close()
    for s, row in zip(sets[:3], t0):
        assert np.array_equal(row, lt.spread_trials_lt(n, pairs, directed, weight, s, 130, 11, None))
    messy = pairs[rng.permutation(len(pairs))]
    if not directed:
        messy[::2] = messy[::2, ::-1]
    messy = np.concatenate([messy, messy[:100], np.column_stack([np.arange(50), np.arange(50)])])
    dp, dw = arc.as_directed(pairs, directed, weight)
    keep = dw != 0
    W = sp.csr_matrix((dw[keep], (dp[keep, 0], dp[keep, 1])), shape=(n, n))
    b = InfluenceGraph(messy, n=n, directed=directed)
    assert np.array_equal(b.arcs, pairs) and np.array_equal(b.lt_weights(W), weight)
    hops = b._hops(None)
    assert b._native_p(b._resolve(gr.linear_threshold(W))) == LT
    assert np.array_equal(t0, b._ic.spread(sets, LT, 130, 11, hops, per_trial=True)[1])
    for step in (1, 5):
        parts = [b._ic.spread(sets[i:i + step], LT, 130, 11, hops, per_trial=True)[1] for i in range(0, len(sets), step)]
        assert np.array_equal(t0, np.concatenate(parts))
    per_set = n * (3 * 8 * 3 + 4 + 1 + 3 * 4)
    b._ic.set_memory_budget(6 * per_set)   # 20 sets in four chunks of up to six
    assert lc.ic_sets_per_chunk(6 * per_set, n, 3, len(sets)) == 6
    assert np.array_equal(t0, b._ic.spread(sets, LT, 130, 11, hops, per_trial=True)[1])
    b._ic.set_memory_budget(1)             # one set per chunk
    assert np.array_equal(t0, b._ic.spread(sets, LT, 130, 11, hops, per_trial=True)[1])
    order = rng.permutation(len(dp))       # the pairs of the table in another order give the same table
    b._ic.set_lt_weights(dp[order], dw[order])
    assert np.array_equal(t0, b._ic.spread(sets, LT, 130, 11, hops, per_trial=True)[1])
    b.close()


@pytest.mark.parametrize("hops", [None, 2])
def test_marginal_mode(hops):
    n, pairs, directed = _graph("gnp300")
    weight = _weights("gnp300", "uniform")
    g = _native_graph("gnp300", "uniform")
    base = [3, 10, 10, 77]
    cands = [[1], [3], [200], [], [5, 6]]
    _, marg = g.spread(cands, LT, 130, 5, -1 if hops is None else hops, base=base, per_trial=True)
    g.close()
    alone = lt.spread_trials_lt(n, pairs, directed, weight, base, 130, 5, hops)
    for c, row in zip(cands, marg):
        assert np.array_equal(row, lt.spread_trials_lt(n, pairs, directed, weight, base + c, 130, 5, hops) - alone), c
    assert marg.any()


def _same(coll, want):
    indptr, members, roots = want
    assert coll.n_sets == len(roots) and coll.n_members == len(members)
    assert np.array_equal(coll.roots, roots)
    assert np.array_equal(coll.indptr, indptr)
    assert np.array_equal(coll.members, members)


@pytest.mark.parametrize("hops", [None, 2])
@pytest.mark.parametrize("name", ["gnp300", "out3", "star130"])
def test_rr_sets_equal_the_restatement(name, hops):
    n, pairs, directed = _graph(name)
    weight = _weights(name, "mixed" if name != "star130" else "uniform")
    spec = gr.linear_threshold(weight)
    g = InfluenceGraph(pairs, n=n, directed=directed)
    for count in (1, 64, 200):                   # default trials and roots: one root pushes, 200 of them pull
        coll = g.rr_sets(count, spec, hops, SEED)
        f = ref.Frontiers()
        _same(coll, lt.rr_sets_lt(n, pairs, directed, weight, count, SEED, hops, frontiers=f))
        if count != 64:
            assert (f.entries()[0] >= lc.ic_pull_min(lc.defines(), 1, n)) == (count == 200)
        assert np.diff(coll.indptr).max() <= (n if hops is None else hops + 1)
        if count != 200:
            coll.close()
    coll.extend(70)                              # the collection's own table, trials 200 ..
    _same(coll, lt.rr_sets_lt(n, pairs, directed, weight, 270, SEED, hops))
    coll.close()
    rng = np.random.default_rng(3)
    trials = rng.integers(0, 2 ** 40, 130).astype(np.uint64)
    trials[5:9] = trials[4]
    roots = rng.integers(0, n, 130)
    roots[6] = roots[5]
    roots[10:14] = 0                             # the hub of a star: its whole row is walked backwards
    coll = g.rr_sets(130, spec, hops, SEED, trials=trials, roots=roots)
    _same(coll, lt.rr_sets_lt(n, pairs, directed, weight, seed=SEED, max_hops=hops, trials=trials, roots=roots))
    coll.close()
    few = np.arange(3, dtype=np.uint64)          # one root entry: round 1 pushes, backwards over vertex 0's whole row
    coll = g.rr_sets(3, spec, hops, SEED, trials=few, roots=np.zeros(3, dtype=np.int64))
    _same(coll, lt.rr_sets_lt(n, pairs, directed, weight, seed=SEED, max_hops=hops, trials=few, roots=np.zeros(3, dtype=np.int64)))
    coll.close()
    g.close()


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("hops", [None, 2])
def test_rr_identity_on_the_device(directed, hops):
    """n samples on trial t, one per root: count_hit(S) = the per-trial spread of S, both from the kernels."""
    name = "out3" if directed else "gnp300"
    n, pairs, _ = _graph(name)
    spec = gr.linear_threshold(_weights(name, "mixed"))
    g = InfluenceGraph(pairs, n=n, directed=directed)
    sets = [[0, 5, 5, 77], list(range(3, n, 41))]
    spread = [g.spread(s, spec, 65, hops, SEED, return_trials=True)[1] for s in sets]
    for t in (0, 64):
        coll = g.rr_sets(n, spec, hops, SEED, trials=np.full(n, t, dtype=np.uint64), roots=np.arange(n))
        for s, counts in zip(sets, spread):
            assert coll.count_hit(s) == counts[t]
        coll.close()
    g.close()
    assert max(c.max() for c in spread) > 4


def _plain_greedy(n, pairs, directed, weight, k, T, hops, seed):
    cache = {}

    def f(s):
        key = tuple(sorted(set(s)))
        if key not in cache:
            cache[key] = int(lt.spread_trials_lt(n, pairs, directed, weight, list(key), T, seed, hops).sum())
        return cache[key]
    seeds = []
    for _ in range(k):
        base = f(seeds)
        gains = [f(seeds + [v]) - base if v not in seeds else -1 for v in range(n)]
        seeds.append(int(np.argmax(gains)))
    return seeds


@pytest.mark.parametrize("directed", [False, True])
def test_greedy(directed):
    n = 60
    raw = np.random.default_rng(5).integers(0, n, (150, 2))
    g = InfluenceGraph(raw, n=n, directed=directed)
    uploads = []
    upload = g._ic.set_lt_weights
    g._ic.set_lt_weights = lambda pairs, weight: (uploads.append(len(weight)), upload(pairs, weight))
    spec = gr.linear_threshold()
    lazy, evals = g.greedy(4, p=spec, n_trials=64, seed=9)
    plain, evals_plain = g.greedy(4, p=spec, n_trials=64, seed=9, celf=False)
    assert len(uploads) == 1   # one specification, one upload: every evaluation of both runs reused the table
    weight = g.lt_weights(spec)
    g.close()
    assert lazy == plain == _plain_greedy(n, g.arcs, directed, weight, 4, 64, None, 9)
    assert evals <= evals_plain


def test_ris_is_max_coverage_of_the_restated_sets():
    n = 200
    raw = np.random.default_rng(6).integers(0, n, (700, 2))
    g = InfluenceGraph(raw, n=n)
    spec = gr.linear_threshold()
    seeds, info = gr.ris_seed_selection(g, 5, p=spec, n_samples=2000, seed=4)
    uploads = []
    upload = g._ic.set_lt_weights
    g._ic.set_lt_weights = lambda pairs, weight: (uploads.append(len(weight)), upload(pairs, weight))
    opim, opim_info = gr.ris_seed_selection(g, 5, p=spec, epsilon=0.5, max_samples=600, seed=4)
    weight = g.lt_weights()
    g.close()
    assert uploads == [] and len(set(opim)) == 5 and opim_info["samples"] <= 600
    indptr, members, _ = lt.rr_sets_lt(n, g.arcs, False, weight, 2000, 4, 198)
    want, gains = ris.max_coverage(indptr, members, n, 5)
    assert seeds == want and info["covered"] == gains.sum() and info["samples"] == 2000


def test_tables_coexist():
    """The Linear Threshold table, then a per-arc table: each of the three models equals its own restatement whichever
    table was set last."""
    n, pairs, directed = _graph("gnp300")
    weight = _weights("gnp300", "mixed")
    prob = arc.mixed_probabilities(np.random.default_rng(1), (len(pairs), 2), 0.3)
    sets = [[1], [3, 50, 50], list(range(0, n, 11))]
    want = {"lt": [lt.spread_trials_lt(n, pairs, directed, weight, s, 70, SEED, 3) for s in sets],
            "arcs": [arc.spread_trials_arcs(n, pairs, directed, prob, s, 70, SEED, 3) for s in sets],
            "p": [ref.spread_trials(n, pairs, directed, s, 0.2, 70, SEED, 3) for s in sets]}
    g = _native.ICGraph(n, pairs, directed)

    def check(kinds):
        for kind in kinds:
            got = g.spread(sets, {"lt": LT, "arcs": None, "p": 0.2}[kind], 70, SEED, 3, per_trial=True)[1]
            assert np.array_equal(got, np.array(want[kind])), kind
    g.set_lt_weights(*arc.as_directed(pairs, directed, weight))
    check(["lt", "p"])
    g.set_arc_probabilities(*arc.as_directed(pairs, directed, prob))
    check(["lt", "arcs", "p", "lt"])
    g.set_lt_weights(*arc.as_directed(pairs, directed, weight))
    check(["arcs", "lt", "p"])
    rr = _native.RRSets(n)
    g.rr_sample(rr, 100, LT, SEED, 2)
    g.rr_sample(rr, 30, None, SEED, 2)
    g.rr_sample(rr, 20, 0.2, SEED, 2)
    indptr, members, _ = rr.download()
    a = lt.rr_sets_lt(n, pairs, directed, weight, 100, SEED, 2)
    b = arc.rr_sets_arcs(n, pairs, directed, prob, seed=SEED, max_hops=2, trials=np.arange(100, 130, dtype=np.uint64))
    c = ris.rr_sets(n, pairs, directed, 0.2, seed=SEED, max_hops=2, trials=np.arange(130, 150, dtype=np.uint64))
    assert np.array_equal(members, np.concatenate([a[1], b[1], c[1]]))
    assert np.array_equal(np.diff(indptr), np.concatenate([np.diff(a[0]), np.diff(b[0]), np.diff(c[0])]))
    rr.close()
    g.close()


def test_public_entry_points_take_linear_threshold():
    G = nx.gnm_random_graph(80, 240, seed=2)
    n, pairs, _, _ = gr.influence._graph_arcs(G)
    uni = gr.lt_weights(pairs, n, False)
    spec = gr.linear_threshold()
    value, iters = gr.ndlib_estimated_influence(G, [0, 7], p=spec, iterations_count=30, n_trials=64, seed=5)
    assert iters == 30 and value == lt.spread_trials_lt(n, pairs, False, uni, [0, 7], 64, 5, 28).mean()
    mixed = lt.mixed_weights(2, n, pairs, False)
    mean, trials = gr.influence_spread(G, [0, 7], p=gr.linear_threshold(mixed), n_trials=64, seed=5, return_trials=True)
    assert np.array_equal(trials, lt.spread_trials_lt(n, pairs, False, mixed, [0, 7], 64, 5, None)) and mean == trials.mean()
    seeds, total = gr.greedy_seed_selection(G, 2, p=spec, n_trials=32, seed=1)
    assert len(set(seeds)) == 2 and total > 0
    seeds, info = gr.ris_seed_selection(G, 3, p=spec, n_samples=500, seed=1)
    assert len(set(seeds)) == 3 and info["samples"] == 500
    g = InfluenceGraph(G)
    assert g.spread([0, 7], spec, 64, 28, 5) == value
    totals = g.marginal_totals([0], [7, 9], spec, 64, None, 5)
    want0 = lt.spread_trials_lt(n, pairs, False, uni, [0], 64, 5, None).sum()
    assert totals.tolist() == [lt.spread_trials_lt(n, pairs, False, uni, [0, c], 64, 5, None).sum() - want0 for c in (7, 9)]
    assert len(g.greedy(2, spec, 32, None, 1)[0]) == 2
    coll = g.rr_sets(10, spec, None, 5)
    coll.extend(5)
    _same(coll, lt.rr_sets_lt(n, pairs, False, uni, 15, 5, None))
    coll.close()
    g.close()
    with pytest.raises(ValueError):
        gr.influence_spread(G, [0], p=gr.linear_threshold("wc"))
    with pytest.raises(ValueError):
        gr.influence_spread(G, [0], p=gr.linear_threshold(np.full(len(pairs), 0.9)))


def test_run_influence_benchmark_linear_threshold():
    res = gr.run_influence_benchmark(gr.planted_partition_edges, {"n": 200, "communities": 4, "deg_in": 6, "deg_out": 1},
                                     k=5, p=gr.linear_threshold(), iterations=50, num_layout_iterations=5, ris=True)
    keys = {"graph_type", "n", "m", "backend", "graphem_seeds", "greedy_seeds", "graphem_influence", "greedy_influence",
            "random_influence", "graphem_time", "greedy_time", "graphem_eval_time", "greedy_eval_time",
            "greedy_iterations", "graphem_norm_influence", "greedy_norm_influence", "random_norm_influence",
            "graphem_efficiency", "greedy_efficiency", "total_time", "ris_seeds", "ris_influence", "ris_time", "ris_samples"}
    assert keys <= set(res)
    assert res["n"] == 200 and len(res["greedy_seeds"]) == 5 and len(res["graphem_seeds"]) == 5 and len(res["ris_seeds"]) == 5
    assert 5 <= res["greedy_influence"] <= 200


def test_errors_and_a_failed_set_keeps_the_table():
    n, pairs, directed = _graph("out3")
    weight = _weights("out3", "mixed")
    g = _native.ICGraph(n, pairs, True)
    rr = _native.RRSets(n)
    g.set_arc_probabilities(pairs, np.full(len(pairs), 0.5))     # a per-arc table is no Linear Threshold table
    with pytest.raises(ValueError, match="no Linear Threshold weights"):
        g.spread([[0]], LT, 8)
    with pytest.raises(ValueError, match="no Linear Threshold weights"):
        g.rr_sample(rr, 4, LT)
    assert rr.counts() == (0, 0)
    g.set_lt_weights(pairs, weight)
    _, t0 = g.spread([[1], [2, 3]], LT, 70, SEED, per_trial=True)
    u, v = (int(x) for x in pairs[0])
    absent = next([a, b] for a in range(n) for b in range(n) if a != b and not ((pairs == [a, b]).all(axis=1)).any())
    heavy = int(np.argmax(np.bincount(pairs[:, 1], minlength=n)))
    row = pairs[pairs[:, 1] == heavy]                            # every in-arc of one vertex at weight 0.6
    assert len(row) >= 2
    bad = [([absent], [0.5], "not an arc"), ([[u, u]], [0.5], "not an arc"), ([[u, n]], [0.5], None),
           ([[u, v], [u, v]], [0.5, 0.5], "twice"), ([[u, v]], [np.nan], r"\[0, 1\]"), ([[u, v]], [1.5], r"\[0, 1\]"),
           ([[u, v]], [-0.25], r"\[0, 1\]"), ([[u, v]], [0.5, 0.5], None),
           (row, np.full(len(row), 0.6), f"vertex {heavy} sum"),
           (row[:2], [0.5, 0.5 + 2.0 ** -19], f"vertex {heavy} sum")]
    for bad_pairs, bad_weight, message in bad:
        with pytest.raises(ValueError, match=message):
            g.set_lt_weights(bad_pairs, bad_weight)
        assert np.array_equal(t0, g.spread([[1], [2, 3]], LT, 70, SEED, per_trial=True)[1])   # the old table is in place
    g.set_lt_weights(row[:2], [0.5, 0.5 + 2.0 ** -21])           # inside the margin; and arcs that are not listed get 0
    half = np.arange(len(pairs)) % 2 == 0
    g.set_lt_weights(pairs[half], weight[half])
    _, t1 = g.spread([[1], [2, 3]], LT, 70, SEED, per_trial=True)
    for s, got in zip([[1], [2, 3]], t1):
        assert np.array_equal(got, lt.spread_trials_lt(n, pairs, True, np.where(half, weight, 0.0), s, 70, SEED))
    for kw in (dict(n_trials=0), dict(max_hops=-2)):
        with pytest.raises(ValueError):
            g.spread([[0]], LT, kw.get("n_trials", 8), 0, kw.get("max_hops", -1))
    with pytest.raises(ValueError):
        g.spread([[n]], LT, 8)
    rr.close()
    g.close()
    # an undirected edge is two arcs, each in its own target's row with its own weight
    e = _native.ICGraph(3, [[0, 1], [1, 2]])
    e.set_lt_weights([[0, 1], [1, 0], [2, 1]], [1.0, 0.0, 0.0])
    assert e.spread([[0], [1], [2]], LT, 5).tolist() == [10, 5, 5]   # only 0 -> 1 can be selected (and is, but for 2^-32)
    with pytest.raises(ValueError, match="twice"):
        e.set_lt_weights([[1, 0], [1, 0]], [0.5, 0.5])
    with pytest.raises(ValueError, match="vertex 1 sum"):
        e.set_lt_weights([[0, 1], [2, 1]], [1.0, 1.0])
    e.close()


# ---- past the grid caps (tests/lt_caps.py; tests/test_lt_influence_cpu.py holds the shapes to the sizing rules) ------------
def _same_collection(rr, want):
    indptr, members, roots = rr.download()
    assert rr.counts() == (len(want[2]), len(want[1]))
    assert np.array_equal(roots, want[2])
    assert np.array_equal(indptr, want[0])
    assert np.array_equal(members, want[1])


def _caps_graph(n, pairs, directed, weight):
    g = _native.ICGraph(n, pairs, directed)
    g.set_lt_weights(*arc.as_directed(pairs, directed, weight))
    return g


def test_forward_pull_past_the_cap():
    """17 seed sets on er2000, 1000 trials, uniform weights: 544 816 words of dense state against 524 288 a trip of
    lt_pull_kernel<false>, the last set across the boundary; the frontier passes pull_min from its second level on."""
    s = lc.FWD_PULL
    n, pairs, sets, weight = lt_caps.forward_pull()
    want, _, _ = lt_caps.forward_pull_expected()
    g = _caps_graph(n, pairs, False, weight)
    totals, got = g.spread(sets, LT, s["T"], lt_caps.IC_SEED, -1, per_trial=True)
    again = g.spread(sets[-2:], LT, s["T"], lt_caps.IC_SEED, -1, per_trial=True)[1]
    g.close()
    for j, (row, need) in enumerate(zip(got, want)):
        assert np.array_equal(row, need), f"set {j}"
    assert np.array_equal(totals, want.sum(axis=1))
    assert np.array_equal(again, want[-2:])


def test_forward_push_past_the_cap():
    """8 sets of 1060 seeds, 4033 trials, one hop: 8480 frontier entries stay under pull_min and make 542 720 (entry, word)
    items, a second, partial trip of lt_push_kernel<false>."""
    s = lc.FWD_PUSH
    n, pairs, sets, weight = lt_caps.forward_push()
    want = lt_caps.forward_push_expected()
    g = _caps_graph(n, pairs, True, weight)
    totals, got = g.spread(sets, LT, s["T"], lt_caps.IC_SEED, 1, per_trial=True)
    g.close()
    for j, (row, need) in enumerate(zip(got, want)):
        assert np.array_equal(row, need), f"set {j}"
    assert np.array_equal(totals, want.sum(axis=1))


def test_reverse_push_past_the_cap():
    """8192 samples in one chunk of 128 words, 8000 distinct roots, one hop: 1 024 000 (entry, word) items, two trips of
    lt_push_kernel<true>."""
    s = lc.REV_PUSH
    n, pairs, trials, roots, weight = lt_caps.reverse_push()
    want = lt_caps.reverse_push_expected()
    g = _caps_graph(n, pairs, True, weight)
    rr = _native.RRSets(n)
    g.rr_sample(rr, s["samples"], LT, lt_caps.IC_SEED, 1, trials=trials, roots=roots)
    _same_collection(rr, want)
    rr.close()
    g.close()


def test_reverse_pull_at_the_largest_state_that_pulls():
    """The sizing rules keep lt_pull_kernel<true> within one trip (tests/lt_caps.py): 1024 distinct roots on 16 003 vertices
    at 16 words is the shape that pulls in round 1 -- 256 048 words of dense state, 1001 workgroups -- and pushes later."""
    s = lt_caps.REV_PULL
    n, pairs, roots, weight = lt_caps.reverse_pull()
    want, _ = lt_caps.reverse_pull_expected()
    g = _caps_graph(n, pairs, False, weight)
    rr = _native.RRSets(n)
    g.rr_sample(rr, s["samples"], LT, lt_caps.IC_SEED, s["hops"], roots=roots)
    _same_collection(rr, want)
    rr.close()
    g.close()
