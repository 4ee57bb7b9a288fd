"""Per-arc Independent Cascade without a GPU: influence.arc_probabilities on every accepted form and every error, and the
numpy restatement (tests/arc_ic_reference.py) against the uniform restatement, against the exact moments under
independent coins per directed arc (the header's deferred-decisions claim), and against the RR identity."""
import numpy as np
import pytest
import scipy.sparse as sp

import graphem_rapids_amd as gr
from graphem_rapids_amd.influence import _graph_arcs, arc_probabilities, trivalency_probabilities

import arc_ic_reference as arc
import ic_reference as ref
import ris_reference as ris


def _star(n):
    return np.column_stack([np.zeros(n - 1, dtype=np.int64), np.arange(1, n)])


# ---- arc_probabilities --------------------------------------------------------------------------------------------------

def test_exported_from_the_package():
    assert gr.arc_probabilities is arc_probabilities and gr.trivalency_probabilities is trivalency_probabilities
    assert {"arc_probabilities", "trivalency_probabilities"} <= set(gr.__all__)


@pytest.mark.parametrize("name", ["wc", "weighted_cascade"])
def test_wc_on_a_star(name):
    n, arcs, directed, _ = _graph_arcs(_star(6))
    got = arc_probabilities(arcs, n, directed, name)
    assert got.dtype == np.float64 and got.shape == (5, 2)
    assert np.array_equal(got[:, 0], np.ones(5))          # hub -> leaf: a leaf has degree 1
    assert np.array_equal(got[:, 1], np.full(5, 1.0 / 5))  # leaf -> hub: the hub has degree 5


def test_wc_directed_with_a_zero_indegree_vertex():
    pairs = [[0, 1], [0, 2], [1, 2], [3, 2], [2, 1]]   # nothing enters 0 or 3; vertex 4 is isolated
    n, arcs, directed, _ = _graph_arcs(pairs, n=5, directed=True)
    got = arc_probabilities(arcs, n, directed, "wc")
    assert got.shape == (5,) and np.isfinite(got).all()
    want = {(0, 1): 1 / 2, (0, 2): 1 / 3, (1, 2): 1 / 3, (2, 1): 1 / 2, (3, 2): 1 / 3}
    assert [want[tuple(a)] for a in arcs.tolist()] == got.tolist()


def test_wc_takes_degrees_after_self_loops_and_duplicates_went():
    clean = [[0, 1], [1, 2], [1, 3]]
    messy = clean + [[1, 0], [2, 1], [1, 1], [3, 3], [0, 1]]
    for directed in (False, True):
        n, arcs, _, _ = _graph_arcs(clean, n=4, directed=directed)
        n2, arcs2, _, _ = _graph_arcs(messy if not directed else clean + [[1, 1], [0, 1], [3, 3]], n=4, directed=directed)
        assert np.array_equal(arcs, arcs2)
        assert np.array_equal(arc_probabilities(arcs, n, directed, "wc"), arc_probabilities(arcs2, n2, directed, "wc"))
    n, arcs, _, _ = _graph_arcs(messy, n=4, directed=False)
    assert np.array_equal(arc_probabilities(arcs, n, False, "wc"), [[1 / 3, 1.0], [1.0, 1 / 3], [1.0, 1 / 3]])


def test_arrays_aligned_with_the_arcs():
    n, und, _, _ = _graph_arcs([[0, 1], [2, 1], [0, 3]], n=4)
    n, dirc, _, _ = _graph_arcs([[0, 1], [1, 0], [2, 1]], n=4, directed=True)
    v = [0.25, 0.0, 1.0]
    got = arc_probabilities(dirc, n, True, v)
    assert got.dtype == np.float64 and np.array_equal(got, v)
    assert np.array_equal(arc_probabilities(und, n, False, np.array(v, dtype=np.float32)), np.column_stack([v, v]))
    two = [[0.1, 0.2], [0.3, 0.4], [0.0, 1.0]]
    got = arc_probabilities(und, n, False, two)
    assert got.shape == (3, 2) and np.array_equal(got, two)
    src = np.array(v)
    out = arc_probabilities(dirc, n, True, src)
    out[0] = 0.5
    assert src[0] == 0.25   # the result is the caller's to change


def test_sparse_matrix():
    n, und, _, _ = _graph_arcs([[0, 1], [2, 1], [0, 3]], n=4)          # canonical: (0, 1), (0, 3), (1, 2)
    P = sp.lil_matrix((4, 4))
    P[0, 1], P[1, 0], P[2, 1], P[3, 0] = 0.5, 0.125, 0.75, 1.0
    for form in (sp.csr_matrix, sp.coo_matrix, sp.csc_matrix):
        got = arc_probabilities(und, n, False, form(P))
        assert np.array_equal(got, [[0.5, 0.125], [0.0, 1.0], [0.0, 0.75]])   # an absent entry is 0
    n, dirc, _, _ = _graph_arcs([[0, 1], [1, 0], [2, 1]], n=4, directed=True)
    Q = sp.lil_matrix((4, 4))
    Q[1, 0], Q[2, 1] = 0.25, 1.0
    assert np.array_equal(arc_probabilities(dirc, n, True, sp.csr_matrix(Q)), [0.0, 0.25, 1.0])
    for bad in ((3, 1), (2, 2), (1, 2)):          # not an arc, a self-loop, the reverse of a directed arc
        R = Q.copy()
        R[bad] = 0.5
        with pytest.raises(ValueError, match="not an arc"):
            arc_probabilities(dirc, n, True, sp.csr_matrix(R))
    R = P.copy()
    R[2, 3] = 0.5
    with pytest.raises(ValueError, match="not an arc"):
        arc_probabilities(und, n, False, sp.csr_matrix(R))
    with pytest.raises(ValueError):
        arc_probabilities(und, n, False, sp.csr_matrix((5, 5)))
    for value in (1.5, -0.5, np.nan):
        R = P.copy()
        R[0, 1] = value
        with pytest.raises(ValueError):
            arc_probabilities(und, n, False, sp.csr_matrix(R))


@pytest.mark.parametrize("bad", [
    "uniform", 0.1, None, [0.1, 0.2], [0.1, 0.2, 0.3, 0.4], [0.1, np.nan, 0.3], [0.1, 1.5, 0.3], [0.1, -1e-9, 0.3],
    [[0.1, 0.2, 0.3]], [[0.1, 0.2, 0.3]] * 3, [[0.1, 0.2], [0.3, np.nan], [0.5, 0.6]], [[0.1, 0.2], [0.3, 2.0], [0.5, 0.6]],
    ["a", "b", "c"], np.zeros((3, 2, 1)),
])
def test_everything_else_is_a_value_error_undirected(bad):
    n, und, _, _ = _graph_arcs([[0, 1], [2, 1], [0, 3]], n=4)
    with pytest.raises(ValueError):
        arc_probabilities(und, n, False, bad)


@pytest.mark.parametrize("bad", ["uniform", 0.1, [0.1, 0.2], [0.1, np.nan, 0.3], [0.1, 1.5, 0.3],
                                 [[0.1, 0.2], [0.3, 0.4], [0.5, 0.6]]])   # the last: (A, 2) is for undirected graphs only
def test_everything_else_is_a_value_error_directed(bad):
    n, dirc, _, _ = _graph_arcs([[0, 1], [1, 0], [2, 1]], n=4, directed=True)
    with pytest.raises(ValueError):
        arc_probabilities(dirc, n, True, bad)


def test_trivalency():
    n, und, _, _ = _graph_arcs(gr.erdos_renyi_edges(60, 0.1, seed=1), n=60)
    a = trivalency_probabilities(und, False, seed=4)
    assert a.shape == (len(und), 2) and set(np.unique(a)) == {0.1, 0.01, 0.001}
    assert np.array_equal(a, np.random.default_rng(4).choice((0.1, 0.01, 0.001), size=(len(und), 2)))
    assert np.array_equal(a, trivalency_probabilities(und, False, seed=4))
    assert not np.array_equal(a, trivalency_probabilities(und, False, seed=5))
    d = trivalency_probabilities(und, True, seed=0, values=(0.5, 0.25))
    assert d.shape == (len(und),) and set(np.unique(d)) == {0.5, 0.25}
    assert np.array_equal(arc_probabilities(und, n, False, a), a)   # the result is a specification


# ---- the restatement ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("p,hops", [(0.2, None), (0.45, 2)])
def test_equal_probabilities_give_the_uniform_restatement(directed, p, hops):
    n, T = 300, 130
    raw = np.random.default_rng(11).integers(0, n, (900, 2))
    pairs = ref.canonical_arcs(n, raw, directed)
    prob = np.full(len(pairs) if directed else (len(pairs), 2), p)
    for seeds in ([0], [3, 3, 100, 299], list(range(0, n, 40))):
        got = arc.spread_trials_arcs(n, pairs, directed, prob, seeds, T, 5, hops)
        assert np.array_equal(got, ref.spread_trials(n, raw, directed, seeds, p, T, 5, hops))
    got = arc.rr_sets_arcs(n, pairs, directed, prob, 130, 5, hops)
    for a, b in zip(got, ris.rr_sets(n, raw, directed, p, 130, 5, hops)):
        assert np.array_equal(a, b)


U_EDGES = [[0, 1], [0, 2], [1, 2], [1, 3], [2, 4], [3, 4]]
U_PROB = [[.9, .2], [.5, .7], [.3, .8], [1, .1], [.25, .6], [.4, 0]]
D_ARCS = [[0, 1], [1, 0], [1, 2], [2, 3], [3, 1], [0, 3], [3, 4], [4, 0]]
D_PROB = [.5, .9, .3, .7, .2, .6, 1, .05]
DEFERRED = ([(False, s, h) for s, h in (([0], None), ([4], None), ([1, 4], 1), ([3], 2))] +
            [(True, s, h) for s, h in (([0], None), ([2], None), ([0], 2))])


@pytest.mark.parametrize("directed,seeds,hops", DEFERRED)
def test_shared_coins_have_the_moments_of_independent_coins(directed, seeds, hops):
    """The header's consequence 1: one search tries an undirected edge in at most one direction, so the coin the two
    directions share acts as two independent ones.  mean over T = 65536 trials against the exact mean E and variance Var
    by enumeration of the live-arc subsets: |mean - E| <= 5 sqrt(Var / T).  The runs are deterministic."""
    n, T, seed = 5, 65536, 3
    raw, prob = (D_ARCS, D_PROB) if directed else (U_EDGES, U_PROB)
    pairs = ref.canonical_arcs(n, raw, directed)
    # the probabilities are listed with the arcs as written above; put them into the canonical order
    order = {tuple(a): i for i, a in enumerate(np.asarray(raw).tolist())}
    prob = np.array([prob[order[tuple(a)]] for a in pairs.tolist()], dtype=np.float64)
    trials = arc.spread_trials_arcs(n, pairs, directed, prob, seeds, T, seed, hops)
    E, var = arc.exact_moments(n, *arc.as_directed(pairs, directed, prob), seeds, hops)
    z = (trials.mean() - E) / np.sqrt(var / T)
    print(f"directed={directed} seeds={seeds} hops={hops}: mean {trials.mean():.6f} exact {E:.6f} var {var:.6f} z {z:+.2f}")
    assert abs(trials.mean() - E) <= 5 * np.sqrt(var / T)


def test_exact_moments_on_closed_forms():
    E, var = arc.exact_moments(3, [[0, 1], [1, 2]], [0.5, 0.25], [0])
    assert E == pytest.approx(1 + 0.5 + 0.125) and var == pytest.approx(1 * 0.5 + 4 * 0.375 + 9 * 0.125 - 1.625 ** 2)
    assert arc.exact_moments(3, [[0, 1], [1, 2]], [0.5, 0.25], [0], 1)[0] == pytest.approx(1.5)
    assert arc.exact_moments(3, [[0, 1], [1, 2]], [1.0, 1.0], [1]) == (2.0, 0.0)


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("hops", [None, 2])
def test_rr_identity_on_the_restatement(directed, hops):
    """sum over all roots r of [S meets RR(t, r)] = |R_t(S)|, with asymmetric probabilities on the undirected graph."""
    n, T, seed = 60, 70, 9
    rng = np.random.default_rng(21)
    pairs = ref.canonical_arcs(n, rng.integers(0, n, (150, 2)), directed)
    prob = rng.random(len(pairs) if directed else (len(pairs), 2))
    sets = [[0], [5, 17, 17, 40], list(range(0, n, 9))]
    spread = [arc.spread_trials_arcs(n, pairs, directed, prob, s, T, seed, hops) for s in sets]
    for t in (0, 13, 69):
        indptr, members, _ = arc.rr_sets_arcs(n, pairs, directed, prob, seed=seed, max_hops=hops,
                                              trials=np.full(n, t, dtype=np.uint64), roots=np.arange(n))
        for s, counts in zip(sets, spread):
            assert ris.count_hit(indptr, members, s) == counts[t]
