"""Reverse influence sampling without a GPU: the numpy restatement of the rule (tests/ris_reference.py) against the
identity that ties RR sets to the Independent Cascade counts, closed cases, brute-force maximum coverage, and the OPIM-C
driver of graphem-rapids_amd/influence.py against the exact spread of a graph small enough to enumerate."""
import itertools
import math

import numpy as np
import pytest

from graphem_rapids_amd.influence import InfluenceGraph, RRCollection, opim_c, opim_sample_plan, ris_seed_selection

import ic_reference as ic
import ris_reference as ris


def _multigraph(n, m, seed):
    rng = np.random.default_rng(seed)
    return np.column_stack([rng.integers(0, n, m), rng.integers(0, n, m)])   # self-loops and duplicates included


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.3, 0.5, 1.0])
@pytest.mark.parametrize("hops", [None, 0, 1, 2])
def test_identity_rr_sets_against_spread_counts(directed, p, hops):
    """For a fixed trial t: the roots r whose RR(t, r) meets S number |R_t(S)|."""
    n, seed = 40, 11
    arcs = _multigraph(n, 90, 3)
    S = [4, 17, 4, 30]   # with a duplicate
    want = ic.spread_trials(n, arcs, directed, S, p, 70, seed, hops)
    for t in (0, 5, 69):
        indptr, members, roots = ris.rr_sets(n, arcs, directed, p, seed=seed, max_hops=hops,
                                             trials=np.full(n, t, dtype=np.uint64), roots=np.arange(n))
        assert np.array_equal(roots, np.arange(n))
        assert ris.count_hit(indptr, members, S) == want[t]


def test_directed_path_walks_arcs_backwards():
    arcs = np.array([[0, 1], [1, 2], [2, 3]])
    indptr, members, _ = ris.rr_sets(4, arcs, True, 1.0, trials=[0, 0], roots=[3, 0])
    assert members[indptr[0]:indptr[1]].tolist() == [0, 1, 2, 3]
    assert members[indptr[1]:indptr[2]].tolist() == [0]
    indptr, members, _ = ris.rr_sets(4, arcs, True, 1.0, trials=[0], roots=[3], max_hops=1)
    assert members.tolist() == [2, 3]


def test_default_roots_are_uniform():
    roots = ris.default_roots(7, 5, np.arange(7000))
    counts = np.bincount(roots, minlength=7)
    sigma = math.sqrt(7000 * (1 / 7) * (6 / 7))
    assert len(counts) == 7 and (np.abs(counts - 1000) <= 5 * sigma).all(), counts


def _brute_cover(sets, n, k):
    """Greedy maximum coverage from the definition."""
    covered, seeds, gains = set(), [], []
    for _ in range(min(k, n)):
        best, bg = None, -1
        for v in range(n):
            if v in seeds:
                continue
            g = sum(1 for j, s in enumerate(sets) if j not in covered and v in s)
            if g > bg:
                best, bg = v, g
        seeds.append(best)
        gains.append(bg)
        covered |= {j for j, s in enumerate(sets) if best in s}
    return seeds, gains


def _csr(sets):
    indptr = np.zeros(len(sets) + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(s) for s in sets])
    members = np.array([v for s in sets for v in sorted(s)], dtype=np.int32)
    return indptr, members


def _systems():
    out = {}
    for case in range(4):
        rng = np.random.default_rng(case)
        n = int(rng.integers(5, 30))
        sets = [set(rng.choice(n, int(rng.integers(0, min(n, 6) + 1)), replace=False).tolist())
                for _ in range(int(rng.integers(1, 60)))]
        out[f"random{case}"] = (n, sets)
    out["all_tie"] = (6, [{v} for v in range(6)] * 2)                  # every count 2: picks 0, 1, 2, ...
    out["empty_sets"] = (5, [set(), {3}, set(), {3, 1}, set()])
    out["no_sets"] = (4, [])
    out["covered_early"] = (8, [{2, 5}, {5}, {5, 7}, {2}])            # 5 then 2 cover everything
    return out


@pytest.mark.parametrize("name", sorted(_systems()))
def test_max_coverage_equals_bruteforce(name):
    n, sets = _systems()[name]
    indptr, members = _csr(sets)
    for k in (0, 1, 3, n, n + 5):
        seeds, gains = ris.max_coverage(indptr, members, n, k)
        want_seeds, want_gains = _brute_cover(sets, n, k)
        assert seeds == want_seeds and gains.tolist() == want_gains, (name, k)
        assert len(seeds) == min(k, n)
        assert ris.count_hit(indptr, members, seeds) == sum(want_gains)
    if name == "all_tie":
        assert ris.max_coverage(indptr, members, n, 4)[0] == [0, 1, 2, 3]
    if name == "covered_early":
        seeds, gains = ris.max_coverage(indptr, members, n, 4)
        assert seeds == [5, 2, 0, 1] and gains.tolist() == [3, 1, 0, 0]


# the 10-vertex, 12-edge graph of the stopping-rule test: two 4-cycles with a chord each, joined through 8 and 9
SMALL_N = 10
SMALL_EDGES = np.array([[0, 1], [1, 2], [2, 3], [3, 0], [0, 2], [4, 5], [5, 6], [6, 7], [7, 4], [3, 8], [8, 9], [9, 4]])


def _exact_spreads(p):
    """sigma(S) of every pair S by enumerating all 2^12 live-edge patterns."""
    m = len(SMALL_EDGES)
    q = ic.threshold(p) / 2 ** 24
    pairs = list(itertools.combinations(range(SMALL_N), 2))
    sigma = np.zeros(len(pairs))
    for pattern in range(1 << m):
        reach = [1 << v for v in range(SMALL_N)]
        live = [e for j, e in enumerate(SMALL_EDGES) if pattern >> j & 1]
        changed = True
        while changed:   # at the fixed point every vertex holds its component's mask
            changed = False
            for u, v in live:
                both = reach[u] | reach[v]
                if reach[u] != both or reach[v] != both:
                    reach[u] = reach[v] = both
                    changed = True
        weight = q ** len(live) * (1 - q) ** (m - len(live))
        for i, (a, b) in enumerate(pairs):
            sigma[i] += weight * bin(reach[a] | reach[b]).count("1")
    return {pair: s for pair, s in zip(pairs, sigma)}


@pytest.mark.parametrize("p", [0.2, 0.5])
def test_opim_c_bounds_hold_against_enumeration(p):
    k, eps, delta = 2, 0.3, 0.05
    exact = _exact_spreads(p)
    opt = max(exact.values())
    theta_0, theta_max, i_max, _ = opim_sample_plan(SMALL_N, k, eps, delta)
    assert theta_0 == 28 and theta_max == 1533 and i_max == 6
    for seed in range(20):
        c = ris.Collections(SMALL_N, SMALL_EDGES, False, p, seed)
        seeds, info = opim_c(c.sample, c.cover, c.count, SMALL_N, k, eps, delta)
        sigma = exact[tuple(sorted(seeds))]
        print(p, seed, info, sigma, opt)
        assert c.thetas == [theta_0 << i for i in range(info["rounds"])] and info["samples"] == c.thetas[-1]
        assert info["rounds"] <= i_max
        assert sigma >= (1 - 1 / math.e - eps) * opt
        assert info["lower"] <= sigma
        assert info["upper"] >= opt
        assert info["ratio"] >= 1 - 1 / math.e - eps or info["rounds"] == i_max
        assert info["estimated_influence"] == SMALL_N * info["covered"] / info["samples"]


def test_opim_c_max_samples_and_arguments():
    c = ris.Collections(SMALL_N, SMALL_EDGES, False, 0.2, 1)
    _, info = opim_c(c.sample, c.cover, c.count, SMALL_N, 2, 0.3, 0.05, max_samples=40)
    assert max(c.thetas) <= 40
    assert opim_c(None, None, None, SMALL_N, 0, 0.3)[0] == []
    for eps, delta in ((0.0, 0.1), (1.0, 0.1), (0.3, 0.0), (0.3, 1.0)):
        with pytest.raises(ValueError):
            opim_c(c.sample, c.cover, c.count, SMALL_N, 2, eps, delta)


def test_estimate_agrees_with_monte_carlo():
    n, p, theta, T = 300, 0.05, 20000, 2000
    rng = np.random.default_rng(7)
    upper = np.column_stack(np.triu_indices(n, 1))
    edges = upper[rng.random(len(upper)) < 0.05]
    S = [3, 50, 120, 200, 299]
    indptr, members, _ = ris.rr_sets(n, edges, False, p, theta, seed=21)
    share = ris.count_hit(indptr, members, S) / theta
    estimate = n * share
    trials = ic.spread_trials(n, edges, False, S, p, T, seed=22)
    se = math.hypot(n * math.sqrt(share * (1 - share) / theta), trials.std(ddof=1) / math.sqrt(T))
    print(estimate, trials.mean(), se)
    assert abs(estimate - trials.mean()) <= 5 * se


class _FakeSets:
    def __init__(self):
        self.asked = None

    def cover(self, k):
        return np.array([2, 0][:k], dtype=np.int32), np.array([5, 1][:k], dtype=np.int64)

    def count_hit(self, ids):
        self.asked = [int(v) for v in ids]
        return 3


def _labelled_graph():
    g = InfluenceGraph.__new__(InfluenceGraph)   # no device: the label plumbing only
    g.n, g.labels, g._ic = 3, ["a", "b", "c"], None
    g._index = {"a": 0, "b": 1, "c": 2}
    return g


def test_labels_are_mapped_both_ways():
    g, rr = _labelled_graph(), _FakeSets()
    coll = RRCollection(rr, g, 0.1, -1, 0)
    seeds, gains = coll.cover(2)
    assert seeds == ["c", "a"] and gains.tolist() == [5, 1]
    assert coll.count_hit(["b", "c"]) == 3 and rr.asked == [1, 2]
    seeds, info = ris_seed_selection(g, 2, iterations_count=1, n_samples=10, seed=0)   # nothing is ever removed
    assert seeds == ["a", "b"] and info == {"samples": 0, "covered": 0, "estimated_influence": 0.0, "rounds": 0}
    assert set(ris_seed_selection(g, 5, iterations_count=0, seed=0)[1]) >= {"lower", "upper", "ratio"}
    with pytest.raises(ValueError, match="no vertices|no graph"):
        RRCollection(rr).extend(4)


def test_ris_seed_selection_argument_errors():
    g = _labelled_graph()
    with pytest.raises(ValueError, match="not both"):
        ris_seed_selection(g, 2, n_samples=100, epsilon=0.1)
    with pytest.raises(ValueError, match="n_samples"):
        ris_seed_selection(g, 2, n_samples=0)
    with pytest.raises(ValueError, match="k must be"):
        ris_seed_selection(g, -1, n_samples=10)


def test_collection_handle_follows_the_handle_contract():
    """What tests/test_native_handles_cpu.py asks of every handle class: a failed create raises the module's message and
    owns nothing, close is idempotent, and a handle that is not open refuses every call."""
    from graphem_rapids_amd import _native
    rr = _native.RRSets.__new__(_native.RRSets)
    with pytest.raises(RuntimeError, match="invalid device ordinal 4096"):
        rr.__init__(4, 4096)
    assert rr.handle.value is None
    rr.close()
    rr.close()
    for call in (rr.counts, rr.download, lambda: rr.cover(2), lambda: rr.count_hit([0]), lambda: rr.upload([0, 1], [0]),
                 lambda: rr.set_memory_budget(0)):
        with pytest.raises(ValueError, match="handle is NULL"):
            call()
    with pytest.raises(ValueError, match=r"n must be in \[1, 2\^31\)"):
        _native.RRSets(0)
    assert _native.load().gh_rr_last_error(None).decode().startswith("n must be")
