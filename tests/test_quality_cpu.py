"""Layout quality without a GPU (csrc/quality.hip host path, graphem-rapids_amd/quality.py): the library's crossing test
anchored on the reference's recorded intersection forces, the host path against the restatement of the header's rule
(tests/quality_reference.py) bit for bit, closed forms (star, grid, convex complete graph), rows, symmetry, the
estimator, the Python interface and the errors.

Bounds.  Counts, sums of counts, pair flags and min / max length are integers or single correctly rounded values: equal.
Sum L and sum L^2 against math.fsum: relative 2 * E * 2**-53 -- recursive summation of E non-negative terms in any order
errs by at most (E - 1) * 2**-53 relative, and the factor 2 covers the terms' own roundings.
"""
import functools
import math
import os
import types

import numpy as np
import pytest
import scipy.sparse as sp

import graphem_rapids_amd as gr
from graphem_rapids_amd import _native, quality
import quality_reference as ref
from conftest import GOLDEN_CASES, load_golden

QUAL_SYMBOLS = ["gh_qual_create", "gh_qual_destroy", "gh_qual_last_error", "gh_qual_set_positions", "gh_qual_crossings",
                "gh_qual_pairs", "gh_qual_edge_lengths"]
GRID_E = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1000, 5051]
# two segments with disjoint bounding boxes that cross under the float32 rule (why the kernel does not prune by boxes)
DISJOINT_BOXES = np.array([[0.06998461484909058, 0.06998474150896072], [2.662574529647827, 2.662574291229248],
                           [4.330337047576904, 4.330337047576904], [6.195383548736572, 6.195383548736572]], dtype=np.float32)


# ---- the inputs ------------------------------------------------------------------------------------------------------
def gaussian(E, D=3, seed=0):
    rng = np.random.default_rng(100 + E + seed)
    n = max(4, E // 3)
    return rng.standard_normal((n, D)).astype(np.float32), rng.integers(0, n, (E, 2)).astype(np.int32)


def lattice():
    """Nearly collinear quadruples everywhere: integers 0..5 + 1000 + 1e-4 N(0, 1) in float32; self-loops and duplicates stay."""
    rng = np.random.default_rng(7)
    pos = (rng.integers(0, 6, (400, 2)) + 1000 + 1e-4 * rng.standard_normal((400, 2))).astype(np.float32)
    edges = rng.integers(0, 400, (1500, 2)).astype(np.int32)
    edges[10] = edges[11]
    edges[20, 1] = edges[20, 0]
    return pos, edges


def tiny():
    """The lattice cloud minus 1000, times 1e-11: the products of two orientations are subnormal or underflow to zero."""
    pos, edges = lattice()
    return ((pos - np.float32(1000)).astype(np.float64) * 1e-11).astype(np.float32), edges


def star():
    rng = np.random.default_rng(3)
    return rng.standard_normal((300, 2)).astype(np.float32), np.column_stack([np.zeros(299), np.arange(1, 300)]).astype(np.int32)


def grid_graph(side):
    ids = np.arange(side * side).reshape(side, side)
    edges = np.concatenate([np.column_stack([ids[:, :-1].ravel(), ids[:, 1:].ravel()]),
                            np.column_stack([ids[:-1].ravel(), ids[1:].ravel()])]).astype(np.int32)
    pos = np.column_stack([ids.ravel() % side, ids.ravel() // side]).astype(np.float32)
    return pos, edges


def convex_complete(m=40):
    ang = 2 * np.pi * np.arange(m) / m
    pos = np.column_stack([np.cos(ang), np.sin(ang)]).astype(np.float32)
    i, j = np.triu_indices(m, 1)
    return pos, np.column_stack([i, j]).astype(np.int32)


def golden_c1(key):
    g = load_golden("c1_er1000")
    return g[key], g["edges"]


CASES = {f"gaussian{E}": functools.partial(gaussian, E) for E in GRID_E}
CASES.update({
    "golden_pos_0": functools.partial(golden_c1, "pos_0"), "golden_pos_final": functools.partial(golden_c1, "pos_final"),
    "lattice": lattice, "tiny": tiny, "star": star, "grid30": functools.partial(grid_graph, 30), "convex40": convex_complete,
    "d1": functools.partial(gaussian, 257, 1), "d2": functools.partial(gaussian, 257, 2), "d16": functools.partial(gaussian, 1000, 16),
})
# what is known about a case without the restatement: (total of crossing pairs, largest per-edge count)
KNOWN = {"golden_pos_0": (969054, 1414), "golden_pos_final": (4330494, 3235), "star": (0, 0), "grid30": (0, 0),
         "convex40": (math.comb(40, 4), None), "d1": (0, 0), "gaussian0": (0, None), "gaussian1": (0, 0)}


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement's results for a case, computed once and shared by the CPU and the GPU tests (read-only)."""
    pos, edges = CASES[name]()
    counts = ref.crossing_counts(pos, edges)
    counts.setflags(write=False)
    rng = np.random.default_rng(len(edges))
    E = len(edges)
    pairs = rng.integers(0, E, (2000, 2)).astype(np.int32) if E else np.zeros((0, 2), dtype=np.int32)
    if E:
        pairs[:5, 1] = pairs[:5, 0]   # an edge and itself never cross
    return {"pos": pos, "edges": edges, "counts": counts, "pairs": pairs, "pair_cross": ref.pair_crossings(pos, edges, pairs),
            "lengths": ref.length_sums(pos, edges)}


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def check_lengths(got, want, E):
    assert same_bits(got[:2], want[:2]), (got, want)
    for g, w in zip(got[2:], want[2:]):
        assert abs(g - w) <= 2 * E * 2.0 ** -53 * abs(w), (g, w)


def check_against_restatement(device_id, name):
    """Counts, their sum, pair flags and length statistics of the library (host path or device) == the restatement."""
    r = reference(name)
    pos, edges = r["pos"], r["edges"]
    q = _native.LayoutQuality(edges, len(pos), device_id)
    try:
        q.set_positions(pos)
        counts, total = q.crossings()
        assert counts.dtype == np.int32 and np.array_equal(counts, r["counts"]), name
        assert total == int(r["counts"].sum()) and total % 2 == 0
        assert np.array_equal(q.pairs(r["pairs"]), r["pair_cross"]), name
        check_lengths(q.edge_lengths(), r["lengths"], len(edges))
        # strided rows: the same positions inside a wider buffer
        wide = np.full((len(pos), pos.shape[1] + 3), np.float32(1e30))
        wide[:, :pos.shape[1]] = pos
        q.set_positions(wide, D=pos.shape[1], ld=wide.shape[1])
        assert np.array_equal(q.crossings()[0], r["counts"]), name
        check_lengths(q.edge_lengths(), r["lengths"], len(edges))
    finally:
        q.close()
    if name in KNOWN:
        want_total, want_max = KNOWN[name]
        assert total // 2 == want_total, name
        assert want_max is None or counts.max() == want_max, name


def check_rows(device_id, name="lattice"):
    """Empty, one id, repeats, descending: each result equals the all-edges counts at those ids."""
    r = reference(name)
    E = len(r["edges"])
    q = _native.LayoutQuality(r["edges"], len(r["pos"]), device_id)
    try:
        q.set_positions(r["pos"])
        for rows in ([], [E - 1], [5, 5, 0, 5, E - 1, 0], np.arange(E)[::-1], np.arange(0, E, 7)):
            rows = np.asarray(rows, dtype=np.int32)
            counts, total = q.crossings(rows)
            assert counts.shape == rows.shape and np.array_equal(counts, r["counts"][rows]) and total == r["counts"][rows].sum()
    finally:
        q.close()


def check_estimator(device_id, name="golden_pos_final"):
    r = reference(name)
    E = len(r["edges"])
    for S, seed in ((300, 5), (4096, 0), (1, 2)):
        rows = np.sort(np.random.default_rng(seed).choice(E, min(S, E), replace=False))
        want = ref.estimate(r["counts"][rows], E)
        got = gr.estimate_edge_crossings(r["pos"], r["edges"], sample_size=S, seed=seed, device_id=device_id)
        assert got == pytest.approx(want, rel=1e-12), (S, seed)
    assert ref.estimate(r["counts"][:1], E)[1] == 0.0
    got = gr.estimate_edge_crossings(r["pos"], r["edges"], sample_size=E, device_id=device_id)
    assert got == (r["counts"].sum() // 2, 0.0)
    assert gr.estimate_edge_crossings(r["pos"], r["edges"], sample_size=10 * E, device_id=device_id) == got


# ---- anchored on the reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in GOLDEN_CASES if int(load_golden(c)["D"]) >= 2])
def test_crossing_pairs_are_the_pairs_the_reference_pushed_apart(case):
    """Every recorded step: the candidate pairs (sampled[s], knn[s][c]) with i < j that gh_qual_pairs reports crossing touch
    exactly the vertices with a nonzero recorded intersection force (c1_er1000, step 0: 794 vertices on both sides)."""
    g = load_golden(case)
    edges = g["edges"]
    q = _native.LayoutQuality(edges, int(g["n"]), -1)
    for t in g["steps"]:
        sampled, knn = g[f"sampled_{t}"], g[f"knn_{t}"]
        pairs = np.column_stack([np.repeat(sampled, knn.shape[1]), knn.ravel()]).astype(np.int32)
        pairs = pairs[pairs[:, 0] < pairs[:, 1]]
        q.set_positions(g[f"pos_{t}"])
        crossing = pairs[q.pairs(pairs)]
        ours = np.unique(edges[crossing.ravel()].ravel())
        theirs = np.flatnonzero(g[f"F_inter_{t}"].any(axis=1))
        assert np.array_equal(ours, theirs), (case, int(t))
        if case == "c1_er1000" and t == 0:
            assert len(ours) == 794
    q.close()


# ---- host path == restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_host_path_equals_restatement(name):
    check_against_restatement(-1, name)


def test_double_precision_is_another_rule():
    """On nearly collinear quadruples the same formula in double gives other counts, so a double-precision kernel cannot pass."""
    r = reference("lattice")
    c64 = ref.crossing_counts(r["pos"], r["edges"], dtype=np.float64)
    differing = int((c64 != r["counts"]).sum())
    print(f"\nlattice: float32 and float64 counts differ on {differing} of {len(c64)} edges")
    assert differing >= 100
    t = reference("tiny")
    t64 = ref.crossing_counts(t["pos"], t["edges"], dtype=np.float64)
    print(f"tiny: {t['counts'].sum() // 2} crossings in float32, {t64.sum() // 2} in float64")
    assert t["counts"].sum() != t64.sum() and t["counts"].sum() > 0
    # the tiny cloud is the lattice cloud scaled: in double, scaling by 1e-11 changes nothing but roundings; float32 loses pairs
    assert not np.array_equal(t["counts"], r["counts"])


def test_disjoint_bounding_boxes_can_cross():
    """The case csrc/quality.hip quotes: every x of the first segment lies below every x of the second, and the float32 rule
    says they cross.  A kernel that skipped tiles by bounding boxes would not be exact."""
    pos, edges = DISJOINT_BOXES, np.array([[0, 1], [2, 3]], dtype=np.int32)
    assert pos[:2, 0].max() < pos[2:, 0].min()
    assert ref.crossing_counts(pos, edges).tolist() == [1, 1]
    assert not ref.crossing_counts(pos, edges, dtype=np.float64).any()
    assert gr.edge_crossing_counts(pos, edges, device_id=-1).tolist() == [1, 1]
    assert gr.edge_crossings(pos, edges, device_id=-1) == 1


def test_rows():
    check_rows(-1)


def test_symmetry():
    """What is symmetric and what is not.  Permuting the edge order permutes the counts, and a pair (j, i) gets the flag of
    (i, j): both hold for every input, also the nearly collinear lattice.  Swapping the endpoints of half the edges
    permutes nothing else on a cloud in general position; on the lattice it moves the point the differences are taken
    from, orient(b, a, c) is -orient(a, b, c) only up to rounding, and counts change -- in the restatement as in the
    library, which must follow it there too."""
    r = reference("lattice")
    rng = np.random.default_rng(1)
    perm = rng.permutation(len(r["edges"]))
    assert np.array_equal(gr.edge_crossing_counts(r["pos"], r["edges"][perm], device_id=-1), r["counts"][perm])
    assert np.array_equal(_pairs_of(r["pos"], r["edges"], r["pairs"][:, ::-1]), r["pair_cross"])

    def swapped(edges):
        out = edges.copy()
        swap = rng.random(len(out)) < 0.5
        out[swap] = out[swap][:, ::-1]
        return out

    g = reference("gaussian1000")
    perm = rng.permutation(len(g["edges"]))
    assert np.array_equal(gr.edge_crossing_counts(g["pos"], swapped(g["edges"])[perm], device_id=-1), g["counts"][perm])
    edges = swapped(r["edges"])
    want = ref.crossing_counts(r["pos"], edges)
    print(f"\nlattice: swapping endpoints changes {int((want != r['counts']).sum())} of {len(want)} counts in the restatement")
    assert np.array_equal(gr.edge_crossing_counts(r["pos"], edges, device_id=-1), want)


def _pairs_of(pos, edges, pairs, device_id=-1):
    q = _native.LayoutQuality(edges, len(pos), device_id)
    try:
        q.set_positions(pos)
        return q.pairs(pairs)
    finally:
        q.close()


def test_estimator():
    check_estimator(-1)


# ---- the Python interface --------------------------------------------------------------------------------------------
def test_layout_quality_keys_and_values():
    r = reference("golden_pos_final")
    E = len(r["edges"])
    out = gr.layout_quality(r["pos"], r["edges"], device_id=-1)
    assert list(out) == ["n_edges", "crossings", "crossings_stderr", "crossings_exact", "crossings_per_edge", "min", "max", "mean", "std"]
    assert out["n_edges"] == E and out["crossings"] == 4330494 and out["crossings_exact"] is True and out["crossings_stderr"] == 0.0
    assert out["crossings_per_edge"] == 2 * 4330494 / E
    L = ref.edge_lengths(r["pos"], r["edges"])
    assert out["min"] == L.min() and out["max"] == L.max()
    assert out["mean"] == pytest.approx(L.mean(), rel=1e-12) and out["std"] == pytest.approx(L.std(), rel=1e-9)
    assert gr.edge_length_stats(r["pos"], r["edges"], device_id=-1) == {k: out[k] for k in ("min", "max", "mean", "std")}
    est = gr.layout_quality(r["pos"], r["edges"], exact=False, sample_size=500, seed=3, device_id=-1)
    assert est["crossings_exact"] is False and est["crossings_stderr"] > 0
    assert (est["crossings"], est["crossings_stderr"]) == gr.estimate_edge_crossings(r["pos"], r["edges"], 500, 3, device_id=-1)
    assert abs(est["crossings"] - out["crossings"]) <= 5 * est["crossings_stderr"]
    assert quality.EXACT_MAX_EDGES >= E
    empty = gr.layout_quality(np.zeros((3, 2)), np.zeros((0, 2), dtype=np.int32), device_id=-1)
    assert empty["crossings"] == 0 and empty["crossings_per_edge"] == 0.0 and empty["min"] == math.inf and math.isnan(empty["mean"])


def test_adjacency_input_gives_the_embedders_edge_ids():
    from graphem_rapids_amd.embedder_hip import GraphEmbedderHIP
    r = reference("gaussian1000")
    n = len(r["pos"])
    e = r["edges"][r["edges"][:, 0] != r["edges"][:, 1]]
    adj = sp.csr_matrix((np.ones(2 * len(e)), (np.r_[e[:, 0], e[:, 1]], np.r_[e[:, 1], e[:, 0]])), shape=(n, n))
    fake = types.SimpleNamespace(verbose=False, logger=None)
    theirs = GraphEmbedderHIP._extract_edges_from_adjacency(fake, GraphEmbedderHIP._validate_adjacency(adj))   # pylint: disable=protected-access
    ours = quality._edges_from_adjacency(adj)   # pylint: disable=protected-access
    assert np.array_equal(ours, theirs) and len(ours) < len(e)   # duplicates merged by the matrix
    got = gr.edge_crossing_counts(r["pos"], adj, device_id=-1)
    assert np.array_equal(got, ref.crossing_counts(r["pos"], theirs))
    with pytest.raises(ValueError, match="adjacency of"):
        gr.edge_crossings(r["pos"][:-1], adj, device_id=-1)


def test_embedder_has_no_cpu_device():
    """GraphEmbedderHIP refuses device='cpu', so the embedder form is tested in tests/test_hip_quality.py."""
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gr.GraphEmbedderHIP(sp.csr_matrix(np.ones((3, 3))), device="cpu", verbose=False)
    assert callable(gr.GraphEmbedderHIP.edge_crossings) and callable(gr.GraphEmbedderHIP.layout_quality)


def test_errors():
    pos, edges = gaussian(65)
    n = len(pos)
    with pytest.raises(ValueError, match=r"edge 1 has a vertex id outside \[0, n\)"):
        _native.LayoutQuality([[0, 1], [2, n]], n, -1)
    with pytest.raises(ValueError, match=r"edge 0 has a vertex id outside \[0, n\)"):
        _native.LayoutQuality([[-1, 1]], n, -1)
    assert _native.load().gh_qual_last_error(None).decode().startswith("edge 0 ")
    q = _native.LayoutQuality(edges, n, -1)
    for call in (q.crossings, lambda: q.crossings([0]), lambda: q.pairs([[0, 1]]), q.edge_lengths):
        with pytest.raises(ValueError, match="no positions were set"):
            call()
    with pytest.raises(ValueError, match="D must be at least 1"):
        q.set_positions(np.zeros((n, 0), dtype=np.float32))
    with pytest.raises(ValueError, match="ld = 2 is below D = 3"):
        q.set_positions(np.zeros(n * 3, dtype=np.float32), D=3, ld=2)
    with pytest.raises(ValueError, match="host positions only"):
        q.set_positions_device(4096, 3)
    with pytest.raises(ValueError, match=r"positions must be \(\d+, D\)"):
        q.set_positions(pos[:-1])
    q.set_positions(pos)
    for bad in ([65], [-1], [0, 3, 65]):
        with pytest.raises(ValueError, match=rf"row {len(bad) - 1} has an edge id outside \[0, E\)"):
            q.crossings(bad)
    with pytest.raises(ValueError, match=r"pair 1 has an edge id outside \[0, E\)"):
        q.pairs([[0, 1], [2, 65]])
    with pytest.raises(ValueError, match=r"pair 0 has an edge id outside \[0, E\)"):
        q.pairs([[-1, 1]])
    assert q.crossings()[1] == ref.crossing_counts(pos, edges).sum()   # refused calls change nothing
    q.close()
    q.close()
    for call in (q.crossings, lambda: q.pairs([[0, 1]]), q.edge_lengths, lambda: q.set_positions(pos)):
        with pytest.raises(ValueError, match="handle is NULL"):
            call()
    with pytest.raises(ValueError, match="edges are needed"):
        gr.edge_crossings(pos)
    with pytest.raises(ValueError, match=r"positions must be \(n, D\)"):
        gr.edge_crossings(pos.ravel(), edges, device_id=-1)


def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "graphem_hip.h")).read()
    lib = _native.load()
    for name in QUAL_SYMBOLS:
        assert name + "(" in header, name
        assert name in _native.SYMBOLS, name
        assert hasattr(lib, name), name
    for name in ("quality", "edge_crossing_counts", "edge_crossings", "estimate_edge_crossings", "edge_length_stats", "layout_quality"):
        assert name in gr.__all__ and hasattr(gr, name), name
