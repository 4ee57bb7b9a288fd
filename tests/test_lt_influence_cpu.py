"""The Linear Threshold rule of include/graphem_hip.h on the host: the fixed-point intervals, the numpy restatement
(tests/lt_reference.py) against exact enumeration and against the threshold process itself, the RR identity, lt_weights and
linear_threshold, and the shapes of tests/lt_caps.py.  No GPU."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import graphem_rapids_amd as gr
from graphem_rapids_amd import influence as infl

import cascade_caps as cc
import ic_reference as ic
import launch_caps as lc
import lt_caps
import lt_reference as lt

TOP = 2 ** 32 - 1


def _star_rows(d, w):
    """The intervals of a hub (vertex 0) with in-arcs from 1 .. d."""
    return lt.lt_intervals(d + 1, np.arange(1, d + 1), np.zeros(d, dtype=np.int64), w)


# ---- 1. intervals --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2, 3, 7, 64, 65, 1000])
def test_uniform_rows_end_at_the_top_and_ascend(d):
    src, dst, lo, hi = _star_rows(d, np.full(d, 1.0 / d))
    assert np.array_equal(src, np.arange(1, d + 1)) and (dst == 0).all()
    assert lo[0] == 0 and hi[-1] == TOP
    assert np.array_equal(lo[1:], hi[:-1]) and (hi > lo).all()
    off = np.abs((hi - lo).astype(np.int64) - 2.0 ** 32 / d)
    assert off[:-1].max(initial=0.0) <= 1.0 and off[-1] <= 2.0   # two roundings of half a unit each; the clamp takes one more


def test_zero_weights_give_empty_intervals():
    w = np.array([0.0, 0.25, 0.0, 0.0, 0.5, 0.0])
    _, _, lo, hi = _star_rows(6, w)
    assert np.array_equal(hi - lo, (w * 2.0 ** 32).astype(np.uint64))
    assert np.array_equal(hi, np.array([0, 1, 1, 1, 3, 3], dtype=np.uint64) << np.uint64(30))


def test_rows_whose_float_sum_is_not_one_pass():
    for w in (np.full(10, 0.1), np.full(3, 1.0 / 3.0)):
        _, _, lo, hi = _star_rows(len(w), w)
        assert hi[-1] == TOP and (hi > lo).all()
    # d copies of fl(1 / d): the sequential sum stays within the derived margin for every d tried
    for d in (3, 7, 49, 1000, 9973):
        assert _star_rows(d, np.full(d, 1.0 / d))[3][-1] == TOP


def test_a_row_above_the_margin_raises():
    _star_rows(2, [0.5, 0.5 + 2.0 ** -21])                     # 1 + 2^-21: inside the margin, clamped
    assert _star_rows(2, [0.5, 0.5 + 2.0 ** -21])[3][-1] == TOP
    with pytest.raises(ValueError, match="vertex 0"):
        _star_rows(2, [0.5, 0.5 + 2.0 ** -19])
    for bad in ([0.5, float("nan")], [-0.1, 0.2], [1.5, 0.0]):
        with pytest.raises(ValueError):
            _star_rows(2, bad)
    with pytest.raises(ValueError, match="twice"):
        lt.lt_intervals(3, [1, 1], [0, 0], [0.1, 0.1])


def test_intervals_do_not_depend_on_the_order_of_the_pairs():
    rng = np.random.default_rng(5)
    n = 40
    pairs = ic.canonical_arcs(n, rng.integers(0, n, (300, 2)), True)
    w = lt.mixed_weights(3, n, pairs, True)
    want = lt.lt_intervals(n, pairs[:, 0], pairs[:, 1], w)
    for _ in range(3):
        perm = rng.permutation(len(pairs))
        got = lt.lt_intervals(n, pairs[perm, 0], pairs[perm, 1], w[perm])
        assert all(np.array_equal(a, b) for a, b in zip(got, want))


def test_mixed_table_has_every_kind_of_row():
    n = 40
    pairs = ic.canonical_arcs(n, np.random.default_rng(5).integers(0, n, (300, 2)), True)
    w = lt.mixed_weights(3, n, pairs, True)
    src, dst, lo, hi = lt.rows_of(n, pairs, True, w)
    order = np.lexsort((pairs[:, 0], pairs[:, 1]))
    ws = w[order]
    total = np.bincount(dst, weights=ws, minlength=n)
    assert (total == 1.0).any() and ((total > 0) & (total < 0.6)).any() and (ws == 0.0).any() and (ws == 1.0).any()
    tiny = ws == 2.0 ** -33
    assert (tiny & (hi == lo)).any() and (tiny & (hi == lo + 1)).any()   # a positive weight with an empty interval, and one with [0, 1)
    last = np.r_[dst[1:] != dst[:-1], True]
    assert (hi[last & (total[dst] == 1.0)] == TOP).all() and (hi[last & (total[dst] < 0.6)] < TOP).all()


# ---- 2, 3. the restatement against exact enumeration and against the threshold process -------------------------------------
TINY = [(0, 1, .5), (2, 1, .5), (0, 2, .3), (1, 2, .3), (3, 2, .4), (1, 3, 1 / 3), (2, 3, 1 / 3), (4, 3, 1 / 3), (3, 4, .2), (5, 4, .1),
        (4, 5, 1), (5, 6, .6), (0, 6, .25), (6, 0, .05)]
CASES = [(seeds, hops) for seeds in ((0,), (4,), (0, 5)) for hops in (None, 1, 2)]
T_STAT = 16384


@functools.lru_cache(maxsize=None)
def _tiny():
    """(pairs, weight, rows, {case: (mean, std)})."""
    table = {(u, v): w for u, v, w in TINY}
    pairs = np.array(sorted(table), dtype=np.int64)
    weight = np.array([table[tuple(p)] for p in pairs])
    rows = lt.rows_of(7, pairs, True, weight)
    return pairs, weight, rows, {c: lt.exact_moments(7, rows, c[0], c[1]) for c in CASES}


def test_exact_means_are_the_documented_ones():
    moments = _tiny()[3]
    means = [m for m, _ in moments.values()]
    assert abs(moments[((0,), None)][0] - 2.974) < 5e-4 and abs(moments[((0, 5), 1)][0] - 3.75) < 5e-4
    assert abs(min(means) - 2.05) < 5e-3 and abs(max(means) - 4.61) < 5e-3


@pytest.mark.parametrize("case", CASES, ids=str)
def test_restatement_against_exact_enumeration(case):
    pairs, weight, _, moments = _tiny()
    mu, sigma = moments[case]
    got = lt.spread_trials_lt(7, pairs, True, weight, case[0], T_STAT, 7, case[1])
    z = (got.mean() - mu) / (sigma / np.sqrt(T_STAT))
    print(case, "mean", got.mean(), "exact", mu, "z", z)
    assert abs(got.mean() - mu) <= 5.0 * sigma / np.sqrt(T_STAT)


def test_live_edge_search_equals_the_threshold_process():
    """Kempe et al., Claim 2.6, numerically: the threshold process after h rounds against the exact live-edge moments at h
    hops, the nine cases in order on one generator."""
    _, _, rows, moments = _tiny()
    rng = np.random.default_rng(0)
    bad = []
    for case in CASES:
        mu, sigma = moments[case]
        got = lt.threshold_process(7, rows, case[0], case[1], T_STAT, rng)
        z = (got.mean() - mu) / (sigma / np.sqrt(T_STAT))
        print(case, "mean", got.mean(), "exact", mu, "z", z)
        if not abs(got.mean() - mu) <= 5.0 * sigma / np.sqrt(T_STAT):
            bad.append((case, z))
    assert not bad


# ---- 4. the RR identity on the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [True, False])
@pytest.mark.parametrize("hops", [None, 2])
def test_rr_identity_on_the_restatement(directed, hops):
    n, T = 60, 16
    rng = np.random.default_rng(11)
    pairs = ic.canonical_arcs(n, rng.integers(0, n, (200 if directed else 110, 2)), directed)
    weight = lt.mixed_weights(4, n, pairs, directed) if directed else gr.lt_weights(pairs, n, False)
    trials = np.repeat(np.arange(T, dtype=np.uint64), n)
    roots = np.tile(np.arange(n), T)
    indptr, members, _ = lt.rr_sets_lt(n, pairs, directed, weight, seed=9, max_hops=hops, trials=trials, roots=roots)
    sizes = np.diff(indptr)
    assert sizes.min() >= 1 and sizes.max() <= (n if hops is None else hops + 1) and sizes.max() > 1
    for S in ([3], [0, 17, 40], list(range(0, n, 4))):
        want = lt.spread_trials_lt(n, pairs, directed, weight, S, T, 9, hops)
        hit = np.array([np.isin(members[indptr[j]:indptr[j + 1]], S).any() for j in range(len(trials))])
        assert np.array_equal(hit.reshape(T, n).sum(axis=1), want)


# ---- 5. lt_weights and linear_threshold ------------------------------------------------------------------------------------
def test_lt_weights_shapes_and_errors():
    n = 30
    rng = np.random.default_rng(2)
    for directed in (True, False):
        pairs = ic.canonical_arcs(n, rng.integers(0, n, (90, 2)), directed)
        A = len(pairs)
        uni = gr.lt_weights(pairs, n, directed, "uniform")
        assert uni.shape == ((A,) if directed else (A, 2)) and uni.dtype == np.float64
        assert np.array_equal(uni, gr.arc_probabilities(pairs, n, directed, "wc"))
        assert np.array_equal(uni, gr.lt_weights(pairs, n, directed))
        lt.rows_of(n, pairs, directed, uni)                              # and the restatement accepts them
        small = np.full(A, 1.0 / n)
        got = gr.lt_weights(pairs, n, directed, small)
        assert np.array_equal(got, small if directed else np.column_stack([small, small]))
        mixed = lt.mixed_weights(1, n, pairs, directed)
        assert np.array_equal(gr.lt_weights(pairs, n, directed, mixed), mixed)
        arcs, w = cc.arc.as_directed(pairs, directed, mixed)
        W = sp.coo_matrix((w[w > 0], (arcs[w > 0, 0], arcs[w > 0, 1])), shape=(n, n)).tocsr()
        assert np.array_equal(gr.lt_weights(pairs, n, directed, W), mixed)
        # errors
        for bad in (np.full(A, np.nan), np.full(A, -0.5), np.full(A, 1.5), np.zeros(A + 1), np.zeros((A, 3)), 0.1, None, "wc"):
            with pytest.raises(ValueError):
                gr.lt_weights(pairs, n, directed, bad)
        absent = next((u, v) for u in range(n) for v in range(n) if u != v and not ((pairs == (u, v)).all(axis=1).any() or
                                                                                    (pairs == (v, u)).all(axis=1).any()))
        with pytest.raises(ValueError, match="not an arc"):
            gr.lt_weights(pairs, n, directed, sp.coo_matrix(([0.1], ([absent[0]], [absent[1]])), shape=(n, n)))
        with pytest.raises(ValueError):
            gr.lt_weights(pairs, n, directed, sp.coo_matrix((n + 1, n + 1)))
        heavy = int(np.argmax(np.bincount(pairs[:, 1], minlength=n)))     # a vertex with at least two in-arcs
        over = np.where(pairs[:, 1] == heavy, 0.75, 0.0)
        with pytest.raises(ValueError, match=f"vertex {heavy} "):
            gr.lt_weights(pairs, n, directed, over if directed else np.column_stack([over, np.zeros(A)]))


def test_lt_weights_margin():
    pairs = np.array([[1, 0], [2, 0]])
    assert gr.lt_weights(pairs, 3, True, [0.5, 0.5 + 2.0 ** -21])[1] == 0.5 + 2.0 ** -21
    with pytest.raises(ValueError, match="vertex 0 "):
        gr.lt_weights(pairs, 3, True, [0.5, 0.5 + 2.0 ** -19])


def test_linear_threshold_is_a_specification():
    spec = gr.linear_threshold()
    assert isinstance(spec, infl.LinearThreshold) and spec.w == "uniform" and "uniform" in repr(spec)
    w = np.array([0.25, 0.5])
    assert gr.linear_threshold(w).w is w
    a, b = infl._LTTable(w), infl._LTTable(w.copy())
    assert a.key == b.key != infl._LTTable(w[::-1]).key and not a.weight.flags.writeable


# ---- 6. the shapes of tests/lt_caps.py -------------------------------------------------------------------------------------
def test_forward_pull_shape_passes_the_cap():
    d = lc.defines()
    s = lc.FWD_PULL
    n, _, sets, _ = lt_caps.forward_pull()
    _, entries, touched = lt_caps.forward_pull_expected()
    W = lc.ceil_div(s["T"], 64)
    assert lc.ic_sets_per_chunk(d.IC_DEFAULT_BUDGET, n, W, len(sets)) == len(sets)       # one chunk
    pull_min = lc.ic_pull_min(d, len(sets), n)
    print("entries per level", entries, "touched", touched, "pull_min", pull_min)
    assert entries[0] < pull_min <= max(entries)                      # the first level pushes, a later one pulls
    trip = d.IC_MAX_BLOCKS * d.IC_BLOCK
    dense = len(sets) * n * W
    assert trip < dense < 2 * trip and (dense - trip) % d.IC_BLOCK != 0   # a second, partial trip of the dense scan


def test_forward_push_shape_passes_the_cap():
    d = lc.defines()
    s = lc.FWD_PUSH
    n, _, sets, _ = lt_caps.forward_push()
    W = lc.ceil_div(s["T"], 64)
    assert lc.ic_sets_per_chunk(d.IC_DEFAULT_BUDGET, n, W, len(sets)) == len(sets)
    entries = sum(len(np.unique(x)) for x in sets)
    assert entries < lc.ic_pull_min(d, len(sets), n)                  # round 1, the only one, pushes
    trip = d.IC_MAX_BLOCKS * d.IC_BLOCK
    assert trip < entries * W < 2 * trip
    want = lt_caps.forward_push_expected()
    assert want.shape == (len(sets), s["T"]) and want.min() >= s["set_size"] and want.max() > s["set_size"]


def test_reverse_push_shape_passes_the_cap():
    d = lc.defines()
    s = lc.REV_PUSH
    n, _, trials, roots, _ = lt_caps.reverse_push()
    W = lc.rr_words_per_chunk(d, n, s["samples"])
    assert 64 * W >= s["samples"]                                     # one chunk
    entries = len(np.unique(roots))
    assert entries == s["distinct_roots"] < lc.ic_pull_min(d, 1, n)   # round 1, the only one, pushes
    trip = d.IC_MAX_BLOCKS * d.IC_BLOCK
    assert trip < entries * W < 2 * trip
    sizes = np.diff(lt_caps.reverse_push_expected()[0])
    assert sizes.min() == 1 and sizes.max() == 2                      # a root and at most the one source it selects


def test_reverse_pull_cannot_pass_the_cap_and_the_shape_pulls():
    d = lc.defines()
    n_max, W, dense = lt_caps.reverse_pull_reach(d)
    trip = d.IC_MAX_BLOCKS * d.IC_BLOCK
    assert 64 * W >= lc.ic_pull_min(d, 1, n_max) and dense < trip     # the largest graph that can pull fits one trip
    for n in (n_max + 1, 2 * n_max, 100_003, 1_000_003, 2 ** 31 - 1):   # beyond it a frontier of 64 W paths stays in push
        assert 64 * lc.rr_words_per_chunk(d, n, 64 * d.RR_MAX_WORDS) < lc.ic_pull_min(d, 1, n)
    s = lt_caps.REV_PULL
    n = s["n"]
    (indptr, _, _), f = lt_caps.reverse_pull_expected()
    assert lc.rr_words_per_chunk(d, n, s["samples"]) * 64 == s["samples"]
    entries = f.entries()
    print("entries per level", entries, "pull_min", lc.ic_pull_min(d, 1, n))
    assert entries[0] == s["samples"] >= lc.ic_pull_min(d, 1, n)      # round 1 pulls
    assert entries[-1] < lc.ic_pull_min(d, 1, n)                      # and a later one pushes
    assert np.diff(indptr).max() == s["hops"] + 1
