"""k-means, the k-means++ minima, the silhouette sums and cluster recovery without a GPU (csrc/clusters.hip host path,
graphem-rapids_amd/clusters.py) against the restatement of the header's rule (tests/clusters_reference.py).

The comparison rule, used everywhere: labels, counts, n_iter, converged and the BITS of d2 and of the centres must be EQUAL --
the centre update adds integers, so there is nothing to tolerate.  A distance sum of N non-negative terms is held to the
header's (N + 2) 2^-53 relative bound against the restatement's math.fsum (clusters_reference.sums_close) and is exactly 0
when N = 0.

The check_* helpers take the device id: this file runs them on the host path (-1), tests/test_hip_clusters.py on the device."""
import functools
import math
import os
import re

import numpy as np
import pytest

import graphem_rapids_amd as gr
from graphem_rapids_amd import _native, clusters
import clusters_reference as cref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLUSTER_SYMBOLS = ["gh_qual_position_rows", "gh_qual_kmeans_assign", "gh_qual_kmeans", "gh_qual_kmeans_seed_step",
                   "gh_qual_cluster_distance_sums"]
PUBLIC = ["kmeans", "kmeans_plusplus", "nearest_center", "silhouette_samples", "silhouette_score", "cluster_recovery"]
KEYS = ("labels", "centers", "d2", "counts", "inertia", "n_iter", "converged")
NO_EDGES = np.zeros((0, 2), dtype=np.int32)

# n: one vertex, less than a wave, several workgroups, and a size that is no multiple of anything.  D: 1 and 130 take the
# kernel that reads the row from memory, 2 .. 16 the ones that keep it in registers.  k: one tile of centres and several
# (a tile holds 4096 / D centres: 257 > 256 at D = 16), and k = n.
SIZES = [1, 63, 700, 1061]
DIMS = [1, 2, 3, 8, 16]
KS = [1, 2, 7, 64, 65, 257]
CASES = [(n, D, k) for n in SIZES for D in DIMS for k in sorted(set(k for k in KS + [n] if k <= n))]
# the workgroup's bins are in LDS while k (D + 1) <= 2048: 512 clusters at D = 3 are the last that fit, 513 the first that
# add to global memory directly; D = 130 reads rows from memory, D = 4100 reads the centres from memory too (a centre tile is
# 4096 floats)
CASES += [(700, 3, 512), (700, 3, 513), (1061, 7, 256), (1061, 7, 257), (700, 130, 7), (63, 4100, 2), (63, 4100, 7)]


# ---- the inputs ------------------------------------------------------------------------------------------------------
def cloud(n, D, seed=0):
    return np.random.default_rng(900 + n + 31 * D + seed).standard_normal((n, D)).astype(np.float32)


def start_rows(pos, k, seed=0):
    ids = np.sort(np.random.default_rng(seed).choice(len(pos), k, replace=False))
    return pos[ids].copy()


def blobs(seed, k=5, per=60, D=3, spread=30.0):
    """k clusters of `per` points: centres from N(0, spread^2), unit noise.  (positions float32, truth)."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, spread, (k, D))
    truth = np.repeat(np.arange(k), per)
    return (centres[truth] + rng.standard_normal((k * per, D))).astype(np.float32), truth


def gaussians_700():
    """700 points of 7 overlapping Gaussians in the plane, started at the first 7 rows: several updates until it converges."""
    rng = np.random.default_rng(7)
    centres = rng.normal(0.0, 2.0, (7, 2))
    pos = (centres[rng.integers(0, 7, 700)] + rng.standard_normal((700, 2))).astype(np.float32)
    return pos, pos[:7].copy()


@functools.lru_cache(maxsize=None)
def reference(n, D, k):
    """(pos, start, the restatement's k-means) of one case, computed once and shared by the CPU and the GPU tests."""
    pos = cloud(n, D)
    start = start_rows(pos, k)
    want = cref.kmeans(pos, start)
    for a in (pos, start, want["labels"], want["centers"], want["d2"], want["counts"]):
        a.setflags(write=False)
    return pos, start, want


@functools.lru_cache(maxsize=None)
def reference_gaussians(max_iter):
    pos, start = gaussians_700()
    return pos, start, cref.kmeans(pos, start, max_iter)


# ---- the comparison rule ----------------------------------------------------------------------------------------------
def assert_same(got, want, what=""):
    """got: the library's k-means dict (LayoutQuality.kmeans or clusters.kmeans); want: the restatement's or another run's."""
    assert got["labels"].dtype == np.int32 and np.array_equal(got["labels"], want["labels"]), what
    assert got["counts"].dtype == np.int64 and np.array_equal(got["counts"], want["counts"]), what
    assert got["d2"].dtype == np.float32 and cref.same_bits(got["d2"], want["d2"]), what
    assert got["centers"].dtype == np.float32 and cref.same_bits(got["centers"], want["centers"]), what
    assert got["n_iter"] == want["n_iter"] and got["converged"] is bool(want["converged"]), what
    assert int(got["counts"].sum()) == len(got["labels"]), what


def handle(pos, device_id, **kw):
    q = _native.LayoutQuality(NO_EDGES, len(pos), device_id)
    q.set_positions(pos, **kw)
    return q


def native_kmeans(pos, start, device_id, max_iter=300):
    q = handle(pos, device_id)
    try:
        return q.kmeans(start, max_iter)
    finally:
        q.close()


# ---- the checks, by device id -----------------------------------------------------------------------------------------
def check_case(device_id, n, D, k):
    pos, start, want = reference(n, D, k)
    got = gr.kmeans(pos, k, init=start, device_id=device_id)
    assert tuple(got) == KEYS
    assert_same(got, want, (n, D, k))
    assert got["inertia"] == math.fsum(want["d2"].tolist())
    labels, d2 = gr.nearest_center(pos, want["centers"], device_id=device_id)
    assert np.array_equal(labels, want["labels"]) and cref.same_bits(d2, want["d2"])


def check_gaussians(device_id):
    pos, start, want = reference_gaussians(300)
    assert want["converged"] and want["n_iter"] >= 5, "the case is meant to need several updates"
    assert_same(native_kmeans(pos, start, device_id), want)
    for max_iter in (0, 1, 3):
        pos, start, cut = reference_gaussians(max_iter)
        got = native_kmeans(pos, start, device_id, max_iter)
        assert_same(got, cut, max_iter)
        assert got["converged"] is False and got["n_iter"] == max_iter
    # max_iter = 0 is a plain assignment: the start centres come back
    assert cref.same_bits(native_kmeans(pos, start, device_id, 0)["centers"], start)


def corner_cases():
    """name -> (pos, start centres)."""
    rng = np.random.default_rng(11)
    out = {}
    base = cloud(40, 3, seed=1)
    out["duplicated points tie to the lowest centre"] = (np.concatenate([base, base, base[:5]]), np.concatenate([base[:3], base[:3]]))
    out["two equal start centres: the second stays empty"] = (cloud(200, 2, seed=2), np.array([[0.5, 0.5], [0.5, 0.5], [-1, 0]], np.float32))
    out["all-zero positions"] = (np.zeros((50, 3), np.float32), np.zeros((2, 3), np.float32))
    mixed = (rng.choice([-1.0, 1.0], (300, 3)) * 10.0 ** rng.uniform(-20, 6, (300, 3))).astype(np.float32)
    out["1e-20 to 1e6 in one snapshot"] = (mixed, mixed[[0, 50, 100, 150, 200]].copy())
    huge = (rng.choice([-1.0, 1.0], (120, 3)) * rng.uniform(0.5, 2.0, (120, 3)) * 1e30).astype(np.float32)
    out["1e30: d2 overflows"] = (huge, huge[:4].copy())
    halves = np.array([-2.5, -1.5, -0.5, 0.5, 1.5, 2.5, 3.5, -3.5], np.float64) * 2.0 ** -38
    ties = np.zeros((64, 2), np.float32)
    ties[:, 0] = np.tile(halves, 8)
    ties[:, 1] = np.repeat(halves, 8)
    ties[0] = (1.0, -1.0)   # M = 1: s = 38, and q of the others ends in one half
    out["negative halves: ties to even"] = (ties, ties[[1, 30, 63]].copy())
    return out


@functools.lru_cache(maxsize=None)
def reference_corners():
    return {name: (pos, start, cref.kmeans(pos, start)) for name, (pos, start) in corner_cases().items()}


def check_corners(device_id):
    ref = reference_corners()
    for name, (pos, start, want) in ref.items():
        assert_same(native_kmeans(pos, start, device_id), want, name)
    pos, start, _ = ref["duplicated points tie to the lowest centre"]
    first = native_kmeans(pos, start, device_id, 0)                             # start centres 3 .. 5 repeat 0 .. 2 and win nothing
    assert_same(first, cref.kmeans(pos, start, 0))
    assert first["labels"].max() == 2 and not first["counts"][3:].any() and np.all(first["d2"][[0, 1, 2, 40, 41, 42, 80]] == 0)
    pos, start, _ = ref["two equal start centres: the second stays empty"]
    first, second = native_kmeans(pos, start, device_id, 0), native_kmeans(pos, start, device_id, 1)
    assert_same(second, cref.kmeans(pos, start, 1))
    assert first["counts"][0] > 0 and first["counts"][1] == 0                  # empty in the first assignment,
    assert cref.same_bits(second["centers"][1], start[1]) and not cref.same_bits(second["centers"][0], start[0])   # so it keeps its value
    want = ref["all-zero positions"][2]
    assert not want["labels"].any() and not want["centers"].any() and want["converged"]
    want = ref["1e30: d2 overflows"][2]
    lost = np.isinf(want["d2"])
    assert lost.any() and not want["labels"][lost].any() and np.isfinite(want["centers"]).all()
    pos, start, want = ref["negative halves: ties to even"]
    q = np.ldexp(pos.astype(np.float64), 38)
    assert np.any(np.abs(q - np.trunc(q)) == 0.5), "the case is meant to hold exact halves"


def check_permuted_and_strided(device_id):
    pos, start, want = reference(700, 3, 7)
    perm = np.random.default_rng(3).permutation(len(pos))
    got = native_kmeans(pos[perm], start, device_id)
    assert np.array_equal(got["labels"], want["labels"][perm]) and cref.same_bits(got["d2"], want["d2"][perm])
    assert cref.same_bits(got["centers"], want["centers"]) and np.array_equal(got["counts"], want["counts"])
    wide = np.full((len(pos), 5), np.float32(np.nan))   # ld = 5 > D = 3: the padding must not be read
    wide[:, :3] = pos
    q = handle(wide, device_id, D=3, ld=5)
    try:
        assert_same(q.kmeans(start), want)
        assert cref.same_bits(q.position_rows([5, 0, 5]), pos[[5, 0, 5]])
    finally:
        q.close()


def check_refusals(device_id):
    pos = cloud(30, 3)
    for k in (0, -1, 31):
        with pytest.raises(ValueError, match=re.escape("k must be in [1, min(n, 4096)] = [1, 30], got " + str(k))):
            gr.kmeans(pos, k, device_id=device_id)
    big = cloud(5000, 2)
    q = handle(big, device_id)
    try:
        with pytest.raises(ValueError, match=re.escape("k must be in [1, min(n, 4096)] = [1, 4096], got 4097")):
            q.kmeans(big[:4097])
        with pytest.raises(ValueError, match=re.escape("k must be in [1, min(n, 4096)] = [1, 4096], got 4097")):
            q.cluster_distance_sums(np.zeros(5000, np.int32), 4097, [0])
        with pytest.raises(ValueError, match=re.escape("k must be in [1, min(n, 4096)]")):
            gr.kmeans_plusplus(big, 4097, device_id=device_id)
    finally:
        q.close()
    q = handle(pos, device_id)
    try:
        with pytest.raises(ValueError, match="centre 1 is not finite"):
            q.kmeans(np.array([[0, 0, 0], [0, np.nan, 0]], np.float32))
        with pytest.raises(ValueError, match="centre 0 is not finite"):
            q.kmeans_assign(np.array([[np.inf, 0, 0]], np.float32))
        with pytest.raises(ValueError, match=re.escape("label 2 is outside [0, k)")):
            q.cluster_distance_sums(np.r_[0, 1, 2, np.zeros(27)].astype(np.int32), 2)
        with pytest.raises(ValueError, match=re.escape("label 0 is outside [0, k)")):
            q.cluster_distance_sums(np.r_[-1, np.zeros(29)].astype(np.int32), 2)
        with pytest.raises(ValueError, match=re.escape("row 1 has a vertex id outside [0, n)")):
            q.cluster_distance_sums(np.zeros(30, np.int32), 1, [0, 30])
        with pytest.raises(ValueError, match=re.escape("vertex 30 is outside [0, n)")):
            q.kmeans_seed_step(30, True)
        with pytest.raises(ValueError, match="max_iter must be >= 0"):
            q.kmeans(pos[:2], -1)
    finally:
        q.close()
    bad = pos.copy()
    bad[17, 1] = np.nan
    for call in (lambda: gr.kmeans(bad, 2, init=pos[:2], device_id=device_id), lambda: gr.nearest_center(bad, pos[:2], device_id=device_id),
                 lambda: gr.kmeans_plusplus(bad, 2, device_id=device_id),
                 lambda: gr.silhouette_samples(bad, np.arange(30) % 2, device_id=device_id)):
        with pytest.raises(ValueError, match="position row 17 is not finite"):
            call()
    bad[3, 0] = np.inf
    with pytest.raises(ValueError, match="position row 3 is not finite"):
        gr.kmeans(bad, 2, init=pos[:2], device_id=device_id)
    q = _native.LayoutQuality(NO_EDGES, 30, device_id)
    try:
        for call in (lambda: q.kmeans(pos[:2]), lambda: q.kmeans_assign(pos[:2]), lambda: q.kmeans_seed_step(0, True),
                     lambda: q.cluster_distance_sums(np.zeros(30, np.int32), 1), lambda: q.position_rows([0])):
            with pytest.raises(ValueError, match="no positions were set"):
                call()
        q.set_positions(pos)
        with pytest.raises(ValueError, match="no seed step with first set came before"):
            q.kmeans_seed_step(0, False)
        q.kmeans_seed_step(0, True)
        q.kmeans_seed_step(1, False)
        q.set_positions(pos)   # a new snapshot: the running minimum is void
        with pytest.raises(ValueError, match="no seed step with first set came before"):
            q.kmeans_seed_step(2, False)
    finally:
        q.close()
    for labels in (np.zeros(30), np.arange(30)):
        with pytest.raises(ValueError, match="Number of labels is"):
            gr.silhouette_samples(pos, labels, device_id=device_id)
    with pytest.raises(ValueError, match="init must be"):
        gr.kmeans(pos, 2, init="nearest", device_id=device_id)


def check_plusplus(device_id):
    pos = cloud(700, 3)
    for seed in (0, 1, 2, 17):
        want = cref.kmeans_plusplus(pos, 9, seed)
        assert np.array_equal(gr.kmeans_plusplus(pos, 9, seed=seed, device_id=device_id), want), seed
        assert len(set(want.tolist())) == 9
    q = handle(pos, device_id)
    try:
        ids = [5, 600, 5, 44]
        for step, want in enumerate(cref.min_d2_steps(pos, ids)):
            assert cref.same_bits(q.kmeans_seed_step(ids[step], step == 0), want), step
    finally:
        q.close()
    # k = n: a chosen vertex has min_d2 = 0 and is never drawn again, so the ids are a permutation
    small = cloud(20, 2)
    ids = gr.kmeans_plusplus(small, 20, seed=3, device_id=device_id)
    assert sorted(ids.tolist()) == list(range(20)) and np.array_equal(ids, cref.kmeans_plusplus(small, 20, 3))
    # all points coincide: after the first draw the least ids not yet chosen
    same = np.ones((10, 2), np.float32)
    ids = gr.kmeans_plusplus(same, 4, seed=0, device_id=device_id)
    first = int(np.random.default_rng(0).integers(10))
    assert ids.tolist() == [first] + [i for i in range(10) if i != first][:3]
    # the k-means++ start is what kmeans uses: rows of the snapshot at those ids
    got = gr.kmeans(pos, 9, seed=2, device_id=device_id)
    assert_same(got, cref.kmeans(pos, pos[cref.kmeans_plusplus(pos, 9, 2)]))
    ids = np.sort(np.random.default_rng(4).choice(700, 9, replace=False))
    assert_same(gr.kmeans(pos, 9, init="random", seed=4, device_id=device_id), cref.kmeans(pos, pos[ids]))
    # n_init: the least inertia of the seeds seed, seed + 1, ...; the earliest on a tie
    runs = [cref.kmeans(pos, pos[cref.kmeans_plusplus(pos, 9, s)]) for s in (5, 6, 7)]
    inertia = [math.fsum(r["d2"].tolist()) for r in runs]
    got = gr.kmeans(pos, 9, n_init=3, seed=5, device_id=device_id)
    assert got["inertia"] == min(inertia)
    assert_same(got, runs[inertia.index(min(inertia))])


# (n, D, k, rows): 1061 > the 1024-column tile at D = 3, and a tile is 512 columns at D = 16: clusters straddle the
# boundaries; D = 130 does not fit a 64-column tile and reads the columns from memory; rows with repeats and in any order
SUM_CASES = [(63, 2, 3, None), (1061, 3, 7, "sample"), (1061, 16, 5, "sample"), (700, 130, 4, "sample"), (700, 1, 65, "sample")]


@functools.lru_cache(maxsize=None)
def reference_sums(n, D, k, rows):
    pos = cloud(n, D, seed=5)
    labels = np.random.default_rng(n + k).integers(0, k, n).astype(np.int32)
    labels[:k] = np.arange(k)            # every cluster has a member
    labels[labels == k - 1] = 0
    labels[n // 2] = k - 1               # the last cluster is a singleton
    ids = None if rows is None else np.r_[np.random.default_rng(1).integers(0, n, 40), n // 2, n // 2, n - 1, 0]
    return pos, labels, ids, cref.distance_sums(pos, labels, k, ids)


def check_sums(device_id, n, D, k, rows):
    pos, labels, ids, want = reference_sums(n, D, k, rows)
    q = handle(pos, device_id)
    try:
        got = q.cluster_distance_sums(labels, k, ids)
    finally:
        q.close()
    n_terms = cref.terms(labels, k, ids)
    assert got.dtype == np.float64 and cref.sums_close(got, want, n_terms)
    assert np.all(got[n_terms == 0] == 0.0) and (n_terms == 0).any()   # the singleton's own row
    s = gr.silhouette_samples(pos, labels, rows=ids, device_id=device_id)
    ref = cref.silhouette(want, labels, k, ids)
    # s = (b - a) / max(a, b) = 1 - min / max: the two means are each within (N + 3) 2^-53 relative, so the quotient within
    # twice that and a rounding, absolutely
    assert np.all(np.abs(s - ref) <= (2 * (n + 3) + 4) * 2.0 ** -53)
    who = np.arange(n) if ids is None else ids
    assert np.all(s[labels[who] == k - 1] == 0.0)   # alone in its cluster
    if ids is None:
        assert gr.silhouette_score(pos, labels, device_id=device_id) == math.fsum(s.tolist()) / n
        assert gr.silhouette_score(pos, labels, exact=False, sample_size=n, device_id=device_id) == math.fsum(s.tolist()) / n
        sampled = gr.silhouette_score(pos, labels, exact=False, sample_size=20, seed=3, device_id=device_id)
        pick = np.sort(np.random.default_rng(3).choice(n, 20, replace=False))
        assert sampled == math.fsum(s[pick].tolist()) / 20


def check_silhouette_against_sklearn(device_id):
    metrics = pytest.importorskip("sklearn.metrics")
    for n, D, k in ((300, 3, 5), (1061, 16, 7)):
        pos = cloud(n, D, seed=8)
        labels = cref.kmeans(pos, start_rows(pos, k), 5)["labels"]
        got = gr.silhouette_samples(pos, labels, device_id=device_id)
        want = metrics.silhouette_samples(pos.astype(np.float64), labels)
        # the float32 chain gives d2 within (D + 2) 2^-24 relative of the float64 value scikit-learn computes, the distance
        # within half of that; a and b are means of distances, so each is within eps = (D + 2) 2^-24 relative, and
        # s = 1 - min(a, b) / max(a, b) within 2 eps (1 + eps) absolutely; the float64 roundings on both sides are far below
        eps = (D + 2) * 2.0 ** -24
        assert np.all(np.abs(got - want) <= 2 * eps * (1 + eps) + 1e-12), (n, D)
        assert abs(gr.silhouette_score(pos, labels, device_id=device_id) - metrics.silhouette_score(pos.astype(np.float64), labels)) <= 2 * eps * (1 + eps) + 1e-12


# generator seed -> k-means++ seed: pairs for which the restatement alone recovers the blobs exactly
RECOVERY = [(100, 0), (101, 1), (102, 2), (103, 3), (104, 4), (105, 5)]


def check_recovery(device_id):
    for gen, seed in RECOVERY:
        pos, truth = blobs(gen)
        alone = cref.kmeans(pos, pos[cref.kmeans_plusplus(pos, 5, seed)])
        assert gr.adjusted_rand_index(truth, alone["labels"]) == 1.0, "the pair was chosen so that the restatement recovers the blobs"
        got = gr.cluster_recovery(pos, truth, n_init=1, seed=seed, device_id=device_id)
        assert list(got) == ["k", "ari", "nmi", "inertia", "silhouette", "silhouette_exact", "n_iter", "converged", "labels"]
        assert got["k"] == 5 and got["ari"] == 1.0 and got["nmi"] == 1.0 and got["converged"] and got["silhouette_exact"]
        assert np.array_equal(got["labels"], alone["labels"]) and got["n_iter"] == alone["n_iter"]
        assert got["inertia"] == math.fsum(alone["d2"].tolist())
        assert -1.0 <= got["silhouette"] <= 1.0 and got["silhouette"] ==gr.silhouette_score(pos, got["labels"], device_id=device_id)
    pos, truth = blobs(100)
    four = gr.cluster_recovery(pos, truth, n_init=4, seed=0, device_id=device_id)   # the default four starts keep the best
    assert four["ari"] == 1.0 and four["nmi"] == 1.0
    coarse = gr.cluster_recovery(pos, truth, k=2, device_id=device_id)
    assert coarse["k"] == 2 and coarse["ari"] < 1.0 and 0.0 < coarse["nmi"] < 1.0


# ---- the host path ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D,k", CASES)
def test_host_path_equals_restatement(n, D, k):
    check_case(-1, n, D, k)


def test_gaussians_and_max_iter_on_the_host_path():
    check_gaussians(-1)


def test_rule_corners_on_the_host_path():
    check_corners(-1)


def test_permuted_and_strided_positions_on_the_host_path():
    check_permuted_and_strided(-1)


def test_refusals_on_the_host_path():
    check_refusals(-1)


def test_kmeans_plusplus_on_the_host_path():
    check_plusplus(-1)


@pytest.mark.parametrize("n,D,k,rows", SUM_CASES)
def test_distance_sums_and_silhouette_on_the_host_path(n, D, k, rows):
    check_sums(-1, n, D, k, rows)


def test_silhouette_against_sklearn_on_the_host_path():
    check_silhouette_against_sklearn(-1)


def test_recovery_of_blobs_on_the_host_path():
    check_recovery(-1)


def test_torch_tensor_positions():
    import torch
    pos, start, want = reference(63, 3, 7)
    assert_same(gr.kmeans(torch.from_numpy(pos.copy()), 7, init=torch.from_numpy(start.copy()), device_id=-1), want)


# ---- normalised mutual information (a host function) -------------------------------------------------------------------
def test_nmi_values():
    rng = np.random.default_rng(0)
    a = rng.integers(0, 6, 5000)
    assert gr.normalized_mutual_info(a, a) == 1.0
    assert gr.normalized_mutual_info(a, (a * 7 + 3) % 11) == 1.0          # a relabelling: the cells are the same
    assert gr.normalized_mutual_info(["x", "y", "x"], [2, 9, 2]) == 1.0
    b = rng.integers(0, 9, 5000)
    indep = gr.normalized_mutual_info(a, b)
    assert 0.0 <= indep < 0.01                                             # independent: MI is about (6 - 1)(9 - 1) / (2 n)
    assert gr.normalized_mutual_info(b, a) == pytest.approx(indep, abs=1e-15)
    perm = rng.permutation(5000)
    relabel = rng.permutation(9)
    assert gr.normalized_mutual_info(a[perm], relabel[b][perm]) == pytest.approx(indep, abs=54 * 2.0 ** -50)
    assert gr.normalized_mutual_info(np.zeros(10), np.zeros(10)) == 1.0   # both trivial
    assert gr.normalized_mutual_info(np.arange(1), np.arange(1)) == 1.0
    assert gr.normalized_mutual_info([], []) == 1.0
    assert gr.normalized_mutual_info(np.zeros(10), np.arange(10)) == 0.0  # one trivial
    with pytest.raises(ValueError, match="same length"):
        gr.normalized_mutual_info([0, 1], [0])
    for x, y in ((a, b), (a[:50], b[:50]), (a % 2, b), (np.arange(40) // 4, np.arange(40) // 5)):
        cells = len(set(zip(x.tolist(), y.tolist())))
        assert abs(gr.normalized_mutual_info(x, y) - cref.nmi(x, y)) <= cells * 2.0 ** -50


def test_nmi_against_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(1)
    for n, ka, kb in ((5000, 6, 9), (300, 5, 5), (64, 2, 30)):
        a, b = rng.integers(0, ka, n), rng.integers(0, kb, n)
        b[: n // 2] = a[: n // 2] % kb   # half dependent
        cells = len(set(zip(a.tolist(), b.tolist())))
        # each cell term carries a few roundings
        assert abs(gr.normalized_mutual_info(a, b) - metrics.normalized_mutual_info_score(a, b)) <= cells * 2.0 ** -50


# ---- plumbing --------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    import ctypes
    header = open(os.path.join(ROOT, "include", "graphem_hip.h")).read()
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in CLUSTER_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert hasattr(lib, name) and name in _native.SYMBOLS, name


def test_public_names():
    assert gr.clusters is clusters and "clusters" in gr.__all__
    for name in PUBLIC:
        assert name in gr.__all__ and getattr(gr, name) is getattr(clusters, name), name
    assert "normalized_mutual_info" in gr.__all__ and gr.normalized_mutual_info is gr.communities.normalized_mutual_info
    assert gr.clustering is gr.graphstats.clustering   # the clustering coefficient keeps its name
    assert clusters.EXACT_MAX_SILHOUETTE_VERTICES > clusters.HOST_EXACT_MAX_SILHOUETTE_VERTICES > 0
