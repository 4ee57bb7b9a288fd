"""Anchors tests/sampler_reference.py -- the vectorised restatement of the device sampler that the float32 engine's own
draws are pinned to in test_hip_device_sampler.py -- without a GPU: against the Python-integer restatement
(f64_reference.sample_ids), and the rule itself against what a sampler owes its caller at the sizes the engine draws on
the device: distinct ids, every id equally likely, iterations and seeds unrelated.

Every figure below is a fixed fact about the rule (seeded, deterministic), measured once and written beside its bound;
the bounds come from the sampling distributions, not from the measurements."""
import functools

import numpy as np
import pytest

import f64_reference
import sampler_reference as sr


@pytest.mark.parametrize("E", sr.GRID_E)
def test_vectorised_form_equals_the_python_integer_form(E):
    S = min(E, 300)
    for seed in sr.GRID_SEEDS:
        for it in sr.GRID_ITERATIONS:
            got = sr.sample_ids(E, S, seed, it)
            assert got.dtype == np.int32 and got.shape == (S,)
            assert np.array_equal(got, f64_reference.sample_ids(E, S, seed, it)), (E, seed, it)


@pytest.mark.parametrize("E", [e for e in sr.GRID_E if e <= sr.GRID_FULL_MAX_E])
def test_full_draw_is_a_permutation(E):
    """S = E: every id once, for every key of the grid (cycle walking neither repeats an id nor leaves one out), and the
    t-th value does not depend on S."""
    want = np.arange(E)
    for seed in sr.GRID_SEEDS:
        for it in sr.GRID_ITERATIONS:
            ids = sr.sample_ids(E, E, seed, it)
            assert np.array_equal(np.sort(ids), want), (E, seed, it)
            assert np.array_equal(ids[:min(E, 300)], sr.sample_ids(E, min(E, 300), seed, it))
    assert np.array_equal(sr.sample_ids(E, E, 0, 0), f64_reference.sample_ids(E, E, 0, 0))


def test_stream_rows_are_the_iterations():
    E, S = 16800, 300
    for seed, t0 in ((0, 0), (12345, 5), ((1 << 64) - 1, (1 << 32) - 2)):
        st = sr.stream(E, S, seed, t0, 4)
        assert st.dtype == np.int32 and st.shape == (4, S)
        for t in range(4):
            assert np.array_equal(st[t], f64_reference.sample_ids(E, S, seed, t0 + t))
    assert sr.stream(E, S, 0, 0, 0).shape == (0, S)


def test_seed_and_iteration_are_taken_modulo_2_64_and_not_less():
    E, S = 16800, 256
    a = sr.sample_ids(E, S, 0, 0)
    assert np.array_equal(a, sr.sample_ids(E, S, 1 << 64, 0)) and np.array_equal(a, sr.sample_ids(E, S, 0, 1 << 64))
    assert not np.array_equal(a, sr.sample_ids(E, S, 1 << 32, 0))      # a key cut to 32 bits would make these collide
    assert not np.array_equal(a, sr.sample_ids(E, S, 0, 1 << 32))
    assert not np.array_equal(sr.sample_ids(E, S, 5, 0), sr.sample_ids(E, S, (1 << 63) + 5, 0))


@functools.lru_cache(maxsize=None)
def _counts(E, S, T):
    st = sr.stream(E, S, 0, 0, T)
    return np.bincount(st.ravel(), minlength=E)


@pytest.mark.parametrize("E,S,T", [(4096, 256, 4096), (16384, 256, 4096), (16385, 256, 4096), (16800, 300, 2000)])
def test_inclusion_is_uniform(E, S, T):
    """How often each id is drawn in iterations 0 .. T - 1 of seed 0.  Under uniform draws without replacement the count of
    an id is Binomial(T, p), p = S / E, and sum_e (c_e - T p)^2 / (T p (1 - p)) is close to chi-square with E - 1 degrees
    of freedom: z, its standardised value, must lie within +-4.  Measured: z = -0.88, 0.66, -0.83, 1.10.  (E = 4096 is
    the floor below which DESIGN.md claims no uniformity; the other three are the sizes around GH_SCAN_MIN_EDGES.)"""
    c = _counts(E, S, T).astype(np.float64)
    assert c.sum() == T * S
    p = S / E
    chi2 = ((c - T * p) ** 2).sum() / (T * p * (1 - p))
    z = (chi2 - (E - 1)) / np.sqrt(2.0 * (E - 1))
    print(f"\nE={E} S={S} T={T}: chi2/df {chi2 / (E - 1):.4f}, z {z:+.2f}; per-id count {int(c.min())}..{int(c.max())} around {T * p:.1f}")
    assert abs(z) <= 4.0, z


def _mean_overlap(rows_a, rows_b):
    return float(np.mean([np.intersect1d(a, b, assume_unique=True).size for a, b in zip(rows_a, rows_b)]))


def test_consecutive_iterations_and_seeds_are_unrelated():
    """Two independent uniform S-subsets of [0, E) share S^2 / E ids on average (here 4), with a standard deviation of
    about 2: the mean of 2000 overlaps has one of about 0.045, and the bound is +-0.25.  Measured: 3.918 for iterations
    t, t + 1 of seed 0; 3.98 for seeds s, s + 1 at iteration 0."""
    E, S, T = 16384, 256, 2000
    want = S * S / E
    st = sr.stream(E, S, 0, 0, T + 1)
    by_iteration = _mean_overlap(st[:-1], st[1:])
    seeds = np.stack([sr.sample_ids(E, S, s, 0) for s in range(T + 1)])
    by_seed = _mean_overlap(seeds[:-1], seeds[1:])
    print(f"\nmean overlap: iterations t, t+1: {by_iteration:.3f}; seeds s, s+1: {by_seed:.3f}; expected {want:.3f}")
    assert abs(by_iteration - want) <= 0.25, by_iteration
    assert abs(by_seed - want) <= 0.25, by_seed


def test_tiny_graphs_are_distinct_but_not_claimed_uniform():
    """E = 33 (three-bit halves): the ids of a draw are distinct, as at every size; inclusion is measurably not uniform
    (S = 8, T = 20000: per-id counts 4678..5179 around 4848, chi^2/df 5.4) and no uniformity is asserted below E = 4096,
    the smallest size tested above -- see DESIGN.md."""
    for it in range(200):
        ids = sr.sample_ids(33, 8, 0, it)
        assert len(np.unique(ids)) == 8 and ids.min() >= 0 and ids.max() < 33
