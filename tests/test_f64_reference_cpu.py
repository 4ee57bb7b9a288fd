"""Anchors tests/f64_reference.py -- the extended-precision iteration the float64 engine is compared with in
tests/test_hip_f64_phases.py -- without a GPU: against what the reference project itself produced computing in float64 (the
*_f64 fixtures of tests/golden), and its sampler and planted inputs against their own claims."""
import os

import numpy as np
import pytest

import f64_reference as reference
from conftest import GOLDEN_DIR


def _rel(a, ref):
    ref = np.asarray(ref, dtype=reference.LD)
    return float(np.abs(np.asarray(a, dtype=reference.LD) - ref).max() / max(1.0, float(np.abs(ref).max())))


@pytest.mark.parametrize("case", ["c1_er1000_f64", "d16_er2000_f64"])
def test_reference_reproduces_every_phase_of_the_float64_fixtures(case):
    """Every captured step: spring forces <= 1e-13 and intersection forces <= 1e-12 relative to max(1, max|ref|), next
    positions <= 1e-10, neighbour rows identical (the bars of test_every_phase_and_one_step_in_float64)."""
    g = np.load(os.path.join(GOLDEN_DIR, case + ".npz"))
    k = int(g["k"])
    Lm, ka, ki = (float(x) for x in g["params"])
    edges = g["edges"]
    worst = {"spring": 0.0, "inter": 0.0, "p2": 0.0}
    for t in g["steps"]:
        pos, sampled = g[f"pos_{t}"], g[f"sampled_{t}"]
        assert pos.dtype == np.float64
        Fs = reference.spring_forces(pos, edges, Lm, ka)
        assert Fs.dtype == reference.LD
        worst["spring"] = max(worst["spring"], _rel(Fs, g[f"F_spring_{t}"]))
        mid = reference.midpoints(pos, edges)
        knn = reference.knn_rows(mid.astype(np.float64), sampled, k)
        assert np.array_equal(knn, g[f"knn_{t}"]), f"{case} step {t}: neighbour rows"
        assert reference.knn_gap(mid.astype(np.float64), sampled, k) > 0.0
        Fi = reference.intersection_forces(pos, edges, sampled, knn, ki)
        worst["inter"] = max(worst["inter"], _rel(Fi, g[f"F_inter_{t}"]))
        out = reference.step(pos, edges, sampled, knn, Lm, ka, ki)
        assert np.array_equal(out, reference.update(pos, Fs, Fi))
        worst["p2"] = max(worst["p2"], float(np.abs(out - g[f"pos_next_{t}"]).max()))
    print(f"\n{case}: extended-precision reference vs the fixtures:", worst)
    assert worst["spring"] <= 1e-13 and worst["inter"] <= 1e-12 and worst["p2"] <= 1e-10, worst


def test_reference_zero_length_edge_and_one_component():
    """A zero-length edge exerts no force (0 / 1e-6, not NaN: pt.py:623-629); one component has no crossings."""
    pos = np.array([[1.0, 2.0], [1.0, 2.0], [4.0, 6.0]])
    F = reference.spring_forces(pos, np.array([[0, 1], [1, 2]]), 1.0, 0.2)
    assert np.isfinite(F.astype(np.float64)).all() and np.all(F[0] == 0)
    want = -0.2 * (5.0 + 1e-6 - 1.0) * np.array([3.0, 4.0]) / (5.0 + 1e-6)
    assert np.abs(F[1].astype(np.float64) - want).max() <= 1e-15 and np.array_equal(F[2], -F[1])
    p1, e1, s1, knn1, _ = reference.planted_intersections(1)
    assert not reference.intersection_forces(p1, e1, s1, knn1).any()


@pytest.mark.parametrize("E", [1, 2, 3, 5, 1000, 4097, 131072])
def test_sample_ids_are_a_keyed_permutation(E):
    ids = reference.sample_ids(E, E, 0, 0)
    assert ids.dtype == np.int32 and np.array_equal(np.sort(ids), np.arange(E))
    if E >= 1000:
        S = 64
        a = reference.sample_ids(E, S, 0, 0)
        assert np.array_equal(a, ids[:S])                                   # the t-th value does not depend on S
        assert not np.array_equal(a, np.arange(S))
        assert not np.array_equal(a, reference.sample_ids(E, S, 12345, 0))    # changes with the seed ...
        assert not np.array_equal(a, reference.sample_ids(E, S, 0, 1))        # ... and with the iteration
        assert np.array_equal(a, reference.sample_ids(E, S, 0, 0))
        assert len(np.unique(reference.sample_ids(E, S, 12345, 2))) == S


def test_degree_ladder_holds_its_degrees():
    n, edges = reference.degree_ladder()
    assert 19000 <= n <= 21000 and edges.min() >= 0 and edges.max() < n
    deg = np.bincount(edges.ravel(), minlength=n)
    hist = np.bincount(deg)
    assert hist[0] == reference.LADDER_ISOLATED
    for d in reference.LADDER_DEGREES:
        assert hist[d] >= reference.LADDER_RUN, d
    for d in reference.LADDER_HUBS:
        assert hist[d] == 1, d
    assert set(np.flatnonzero(hist)) == {0, *reference.LADDER_DEGREES, *reference.LADDER_HUBS}
    key = np.sort(edges, axis=1)
    assert len(np.unique(key[:, 0].astype(np.int64) * n + key[:, 1])) == len(edges) and (edges[:, 0] != edges[:, 1]).all()
    assert (edges[:, 0] > edges[:, 1]).any() and (edges[:, 0] < edges[:, 1]).any()          # endpoints swapped
    assert (np.diff(edges[:, 0].astype(np.int64) * n + edges[:, 1]) < 0).any()                  # not sorted


@pytest.mark.parametrize("D", [2, 3, 4, 5, 8, 16, 31, 32])
def test_planted_intersections_hold_what_they_claim(D):
    """Exact integer classification of every listed pair equals the planted numbers, and the floating-point reference
    finds exactly the crossing ones: the GPU comparison cannot go vacuous."""
    pos, edges, sampled, knn, hub = reference.planted_intersections(D)
    assert pos.shape[1] == D and knn.shape == (len(sampled), reference.PLANTED_K) and np.abs(pos[:, :2]).max() <= 64
    counts = reference.classify_planted(pos, edges, sampled, knn, hub)
    assert counts == reference.PLANTED_COUNTS, counts
    assert 4 * counts["crossing"] >= counts["listed"] and counts["hub"] >= 200
    assert min(counts["touching"], counts["collinear"], counts["shared"], counts["i_gt_j"]) >= 1
    i, j = reference.crossing_pairs(pos, edges, sampled, knn)
    assert len(i) == counts["crossing"]
    pairs = set(zip(i.tolist(), j.tolist()))
    assert len(pairs) == counts["crossing"] - 16          # each fan lists two verticals twice
    listed = {(int(s), int(x)) for s, row in zip(sampled, knn) for x in row}
    assert all((b, a) in listed for a, b in pairs)           # every crossing pair is listed from both sides
    F = reference.intersection_forces(pos, edges, sampled, knn, 0.5)
    assert F.any() and not F[len(pos) - 7:].any()
