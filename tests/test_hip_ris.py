"""gh_ic_rr_sample, gh_rr_cover and gh_rr_count_hit against the numpy restatement of their rule (tests/ris_reference.py), id
for id, and against gh_ic_spread through the identity of include/graphem_hip.h; ris_seed_selection on top of them."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":   # the fresh child process of test_fresh_process_leaves_the_state_zeroed
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import graphem_rapids_amd as gr   # noqa: E402
from graphem_rapids_amd import _native   # noqa: E402
from graphem_rapids_amd.influence import InfluenceGraph   # noqa: E402

import ic_reference as ic   # noqa: E402
import ris_reference as ris   # noqa: E402

pytestmark = pytest.mark.gpu


def _path(n):
    return np.column_stack([np.arange(n - 1), np.arange(1, n)])


def _star(n):
    return np.column_stack([np.zeros(n - 1, dtype=np.int64), np.arange(1, n)])


def _directed(n, m, seed):
    rng = np.random.default_rng(seed)
    return np.column_stack([rng.integers(0, n, m), rng.integers(0, n, m)])


@functools.lru_cache(maxsize=None)
def _graph(name):
    """(n with three isolated vertices n-3 .. n-1, arcs, directed), as tests/test_hip_influence.py builds them."""
    n, arcs, directed = {
        "path": lambda: (50, _path(50), False),
        "star": lambda: (300, _star(300), False),           # hub row of 299 arcs: several blocks of 64
        "er2000": lambda: (2000, gr.erdos_renyi_edges(2000, 0.004, seed=1), False),
        "directed": lambda: (1500, _directed(1500, 6000, 4), True),
    }[name]()
    return n + 3, arcs, directed


def _open(name):
    n, arcs, directed = _graph(name)
    return InfluenceGraph(arcs, n=n, directed=directed)


SEED = 7
CASES = [  # (graph, n_samples, p, max_hops): every value of every axis appears
    ("path", 1000, 0.3, None), ("path", 63, 1.0, 1), ("path", 1, 0.05, 3), ("path", 64, 0.0, 0),
    ("star", 65, 0.3, None), ("star", 64, 1.0, 1), ("star", 1000, 0.05, 3), ("star", 1, 1.0, 0),
    ("er2000", 1000, 0.3, None), ("er2000", 63, 0.05, 3), ("er2000", 64, 1.0, None), ("er2000", 65, 0.0, 1),
    ("directed", 1000, 0.3, None), ("directed", 65, 0.05, 1), ("directed", 64, 1.0, 3), ("directed", 1, 0.0, 0),
]


@functools.lru_cache(maxsize=None)
def _want(name, S, p, hops):
    n, arcs, directed = _graph(name)
    return ris.rr_sets(n, arcs, directed, p, S, SEED, hops)


def _same(coll, want):
    indptr, members, roots = want
    assert coll.n_sets == len(coll) == len(roots) and coll.n_members == len(members)
    assert coll.indptr.dtype == np.int64 and coll.members.dtype == np.int32 and coll.roots.dtype == np.int32
    assert np.array_equal(coll.roots, roots)
    assert np.array_equal(coll.indptr, indptr)
    assert np.array_equal(coll.members, members)


@pytest.mark.parametrize("name,S,p,hops", CASES)
def test_rr_sets_cover_and_count_equal_the_restatement(name, S, p, hops):
    g = _open(name)
    coll = g.rr_sets(S, p, hops, SEED)
    want = _want(name, S, p, hops)
    _same(coll, want)
    n = g.n
    for k in (3, 10):
        seeds, gains = coll.cover(k)
        want_seeds, want_gains = ris.max_coverage(want[0], want[1], n, k)
        assert seeds == want_seeds and gains.dtype == np.int64 and np.array_equal(gains, want_gains)
        assert coll.count_hit(seeds) == gains.sum() == ris.count_hit(want[0], want[1], seeds)
    for verts in ([], [0], [n - 1, n - 2], [1, 1, 5, 0, 5], list(range(0, n, 7))):
        assert coll.count_hit(verts) == ris.count_hit(want[0], want[1], verts)
    coll.close()
    g.close()


@pytest.mark.parametrize("name", ["er2000", "directed"])
@pytest.mark.parametrize("p,hops", [(0.05, None), (0.3, 2), (0.3, None), (0.05, 2)])
def test_identity_against_the_spread_kernel(name, p, hops):
    """sum over all roots r of [S meets RR(t, r)] = |R_t(S)|: the new kernels against gh_ic_spread, no numpy search."""
    g = _open(name)
    n = g.n
    sets = [[0, 5, 5, 77], list(range(3, n, 211))]
    spread = [g.spread(s, p, 65, hops, SEED, return_trials=True)[1] for s in sets]
    for t in (0, 5, 64):
        coll = g.rr_sets(n, p, hops, SEED, trials=np.full(n, t, dtype=np.uint64), roots=np.arange(n))
        assert np.array_equal(coll.roots, np.arange(n))
        for s, counts in zip(sets, spread):
            assert coll.count_hit(s) == counts[t]
        coll.close()
    g.close()


def test_explicit_trials_and_roots():
    name, p, hops = "er2000", 0.3, 2
    n, arcs, directed = _graph(name)
    g = _open(name)
    big = np.uint64(2 ** 32 + 12345)
    # one word: duplicate (root, trial) pairs, a root shared across trials, a trial shared across roots, trials >= 2^32
    trials = np.array([3, 3, 3, 9, 4, 4, 4, big, big + np.uint64(2 ** 40), 3], dtype=np.uint64)
    roots = np.array([10, 10, 11, 10, 20, 21, 20, 10, 10, 10])
    coll = g.rr_sets(len(trials), p, hops, SEED, trials=trials, roots=roots)
    _same(coll, ris.rr_sets(n, arcs, directed, p, seed=SEED, max_hops=hops, trials=trials, roots=roots))
    ip, mb = coll.indptr, coll.members
    sets = [mb[ip[j]:ip[j + 1]].tolist() for j in range(len(trials))]
    assert sets[0] == sets[1] == sets[9] and sets[4] == sets[6]
    assert len({tuple(s) for s in sets}) > 3
    # across words too, and appended to a collection that holds sets already
    rng = np.random.default_rng(1)
    more_t, more_r = rng.integers(0, 5, 200).astype(np.uint64), rng.integers(0, 8, 200)
    coll.extend(200, trials=more_t, roots=more_r)
    _same(coll, ris.rr_sets(n, arcs, directed, p, seed=SEED, max_hops=hops, trials=np.concatenate([trials, more_t]),
                            roots=np.concatenate([roots, more_r])))
    # default trials continue at the collection's size; default roots follow the trial
    coll.extend(70)
    t_all = np.concatenate([trials, more_t, np.arange(210, 280, dtype=np.uint64)])
    r_all = np.concatenate([roots, more_r, ris.default_roots(n, SEED, np.arange(210, 280))])
    _same(coll, ris.rr_sets(n, arcs, directed, p, seed=SEED, max_hops=hops, trials=t_all, roots=r_all))
    with pytest.raises(ValueError):
        coll.extend(2, roots=[0, n])
    with pytest.raises(ValueError):
        coll.extend(2, trials=[1])
    coll.close()
    g.close()


def test_results_do_not_depend_on_the_chunk_budget():
    name, S, p, hops = "er2000", 1000, 0.3, None
    g = _open(name)
    g._ic.set_memory_budget(1)   # one word, 64 samples, per chunk
    coll = g.rr_sets(S, p, hops, SEED)
    _same(coll, _want(name, S, p, hops))
    coll.close()
    g.close()


def test_collection_budget_refuses_and_the_handles_stay_usable():
    n, arcs, directed = _graph("star")
    g = _open("star")
    g._ic.set_memory_budget(1)   # 64 samples per chunk
    coll = g.rr_sets(0, 1.0, None, SEED)
    # p = 1: every set is the star's 300 vertices (or one isolated vertex), so a chunk of 64 is some 77 KB: the third
    # chunk outgrows 200 000 bytes, and the two that were appended go again
    coll.set_memory_budget(200000)
    with pytest.raises(MemoryError, match="mean set size"):
        coll.extend(1000)
    assert len(coll) == 0 and coll.n_members == 0
    coll.extend(10)
    _same(coll, ris.rr_sets(n, arcs, directed, 1.0, 10, SEED))
    with pytest.raises(MemoryError, match="mean set size"):
        coll.extend(1000)
    _same(coll, ris.rr_sets(n, arcs, directed, 1.0, 10, SEED))
    coll.set_memory_budget(0)
    coll.extend(90)
    _same(coll, ris.rr_sets(n, arcs, directed, 1.0, 100, SEED))
    want = ic.spread_trials(n, arcs, directed, [0, 4], 0.3, 70, 5)   # the chunk state was left zero
    assert np.array_equal(g.spread([0, 4], 0.3, 70, None, 5, return_trials=True)[1], want)
    coll.close()
    g.close()


def test_directed_path_walks_arcs_backwards():
    g = InfluenceGraph(np.array([[0, 1], [1, 2], [2, 3]]), n=4, directed=True)
    coll = g.rr_sets(2, 1.0, trials=[0, 0], roots=[3, 0])
    assert coll.members[coll.indptr[0]:coll.indptr[1]].tolist() == [0, 1, 2, 3]
    assert coll.members[coll.indptr[1]:coll.indptr[2]].tolist() == [0]
    coll.close()
    g.close()


def _csr(sets):
    indptr = np.zeros(len(sets) + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(s) for s in sets])
    return indptr, np.array([v for s in sets for v in sorted(s)], dtype=np.int32)


SYSTEMS = {
    "all_tie": (12, [{v} for v in range(12)] * 3),
    "empty_sets": (9, [set(), {3}, set(), {3, 1}, set(), {8}]),
    "no_sets": (7, []),
    "giant_and_singletons": (700, [set(range(0, 700, 2))] + [{v} for v in range(1, 700, 2)] + [{5}, {5}, {699}]),
}


@pytest.mark.parametrize("name", sorted(SYSTEMS))
def test_max_coverage_of_uploaded_systems(name):
    n, sets = SYSTEMS[name]
    indptr, members = _csr(sets)
    for k in (0, 1, 10, n, n + 5):
        seeds, gains = gr.max_coverage(indptr, members, n, k)
        want_seeds, want_gains = ris.max_coverage(indptr, members, n, k)
        assert seeds == want_seeds and np.array_equal(gains, want_gains), (name, k)
        assert len(seeds) == min(k, n)
    rr = _native.RRSets(n)
    rr.upload(indptr, members)
    got = rr.download()
    assert np.array_equal(got[0], indptr) and np.array_equal(got[1], members) and (got[2] == -1).all()
    seeds, gains = rr.cover(n)
    assert gains.sum() == rr.count_hit(seeds) == sum(1 for s in sets if s)
    for bad in ([0, 2, 1], [0, 1, 1]):   # members of a set must ascend strictly, and lie in [0, n)
        with pytest.raises(ValueError):
            rr.upload([0, 3], bad)
    with pytest.raises(ValueError):
        rr.upload([0, 1], [n])
    with pytest.raises(ValueError):
        rr.count_hit([n])
    rr.close()


def test_ris_seed_selection_fixed_mode():
    name, theta, k, p = "er2000", 1000, 6, 0.05
    n, arcs, directed = _graph(name)
    g = _open(name)
    seeds, info = gr.ris_seed_selection(g, k, p, iterations_count=5, n_samples=theta, seed=SEED)
    want = ris.rr_sets(n, arcs, directed, p, theta, SEED, 3)
    want_seeds, want_gains = ris.max_coverage(want[0], want[1], n, k)
    covered = int(want_gains.sum())
    assert seeds == want_seeds
    assert info == {"samples": theta, "covered": covered, "estimated_influence": n * covered / theta, "rounds": 1}
    g.close()


SMALL_N = 10
SMALL_EDGES = np.array([[0, 1], [1, 2], [2, 3], [3, 0], [0, 2], [4, 5], [5, 6], [6, 7], [7, 4], [3, 8], [8, 9], [9, 4]])


@pytest.mark.parametrize("p", [0.2, 0.5])
def test_ris_seed_selection_epsilon_mode_follows_the_restatement(p):
    from graphem_rapids_amd.influence import opim_c
    g = InfluenceGraph(SMALL_EDGES, n=SMALL_N)
    for seed in range(3):
        seeds, info = gr.ris_seed_selection(g, 2, p, epsilon=0.3, delta=0.05, seed=seed)
        c = ris.Collections(SMALL_N, SMALL_EDGES, False, p, seed, 198)
        want_seeds, want = opim_c(c.sample, c.cover, c.count, SMALL_N, 2, 0.3, 0.05)
        assert seeds == want_seeds
        assert set(info) == {"samples", "covered", "estimated_influence", "rounds", "lower", "upper", "ratio"}
        for key in ("samples", "covered", "rounds"):
            assert info[key] == want[key]
        for key in ("estimated_influence", "lower", "upper", "ratio"):
            assert info[key] == pytest.approx(want[key], rel=1e-12, abs=0)
    g.close()


def test_run_influence_benchmark_ris_keys():
    params = {"n": 500, "communities": 4, "deg_in": 6, "deg_out": 1}
    kw = dict(k=4, p=0.1, iterations=20, num_layout_iterations=3)
    plain = gr.run_influence_benchmark(gr.planted_partition_edges, params, **kw)
    with_ris = gr.run_influence_benchmark(gr.planted_partition_edges, params, ris=True, **kw)
    extra = {"ris_seeds", "ris_influence", "ris_time", "ris_samples"}
    assert not extra & set(plain)
    assert set(with_ris) == set(plain) | extra
    assert len(set(with_ris["ris_seeds"])) == 4 and with_ris["ris_samples"] > 0 and 4 <= with_ris["ris_influence"] <= 500


def _child():
    """Sampling, extending twice, covering and closing leave the IC handle's chunk state zeroed: the same draw again gives
    the same sets, and gh_ic_spread on the same graph still equals its restatement."""
    n, arcs, directed = _graph("directed")
    g = _open("directed")
    before = _native.live_allocations()
    coll = g.rr_sets(100, 0.3, None, SEED)
    coll.extend(64)
    coll.extend(37)
    _same(coll, ris.rr_sets(n, arcs, directed, 0.3, 201, SEED))
    seeds, gains = coll.cover(5)
    assert coll.count_hit(seeds) == gains.sum()
    coll.close()
    coll.close()
    again = g.rr_sets(201, 0.3, None, SEED)
    _same(again, ris.rr_sets(n, arcs, directed, 0.3, 201, SEED))
    again.close()
    for s, hops in (([0, 9, 700], None), ([3], 2)):
        want = ic.spread_trials(n, arcs, directed, s, 0.3, 130, 11, hops)
        assert np.array_equal(g.spread(s, 0.3, 130, hops, 11, return_trials=True)[1], want)
    g.close()
    assert _native.live_allocations()[0] <= before[0]
    print("child ok")


def test_fresh_process_leaves_the_state_zeroed():
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "child ok" in out.stdout, out.stdout + out.stderr


if __name__ == "__main__":
    _child()
