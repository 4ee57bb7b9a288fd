"""Neighbour ranks and the embedding-quality measures without a GPU (csrc/quality.hip host path, graphem-rapids_amd/quality.py)
against the restatement of the header's rule (tests/neighbors_reference.py): neighbours, the bits of dist2, below and equal
must be EQUAL; the measures are single divisions of exact integers and must be equal too, except the Jaccard mean, a sum
of len(sources) doubles, which is held to len(sources) * 2**-53 relative.

The library cuts a row longer than QUAL_RANK_PIECE = 64 slots into pieces of 64, one wave each on the device; that is the
only place where a row's degree changes the code path, so the ladders below stand on both sides of every multiple of 64
they reach (63 / 64 / 65, 128 / 129, 300, 5000)."""
import functools
import math
import os

import numpy as np
import pytest
import scipy.sparse as sp

import graphem_rapids_amd as gr
from graphem_rapids_amd import _native, quality
import neighbors_reference as ref

RANK_SYMBOLS = ["gh_qual_neighbor_sizes", "gh_qual_neighbor_ranks"]
ARRAYS = ("sources", "indptr", "neighbors", "dist2", "below", "equal")
DIMS = [1, 2, 3, 4, 8, 16, 17, 130]   # 130: no 64-column tile of 130 rows fits the kernel's LDS, so columns are read from memory


# ---- the inputs ------------------------------------------------------------------------------------------------------
def cloud(n, D=3, seed=0):
    return np.random.default_rng(500 + n + 31 * D + seed).standard_normal((n, D)).astype(np.float32)


def random_edges(n, E, seed=0):
    return np.random.default_rng(900 + n + E + seed).integers(0, n, (E, 2)).astype(np.int32)


def no_edges(n):
    return cloud(n), np.zeros((0, 2), dtype=np.int32)


def complete(m):
    i, j = np.triu_indices(m, 1)
    return cloud(m), np.column_stack([i, j]).astype(np.int32)


def star(m=30):
    return cloud(m, 2), np.column_stack([np.zeros(m - 1), np.arange(1, m)]).astype(np.int32)


def path7():
    return np.arange(7, dtype=np.float32)[:, None], np.column_stack([np.arange(6), np.arange(1, 7)]).astype(np.int32)


def grid12():
    """A 12 x 12 grid graph on its integer lattice: equal distances everywhere."""
    ids = np.arange(144).reshape(12, 12)
    edges = np.concatenate([np.column_stack([ids[:, :-1].ravel(), ids[:, 1:].ravel()]),
                            np.column_stack([ids[:-1].ravel(), ids[1:].ravel()])]).astype(np.int32)
    return np.column_stack([ids.ravel() % 12, ids.ravel() // 12]).astype(np.float32), edges


def clones():
    """50 vertices on 5 positions: thresholds of 0 between clones, where only the w != u exclusion keeps u itself out."""
    return cloud(5)[np.arange(50) % 5], random_edges(50, 200)


def identical():
    return np.tile(cloud(1, 4), (40, 1)), random_edges(40, 100)


def ladder(degrees, D=3):
    """Source i gets exactly degrees[i] neighbours, all from a pool of max(degrees) further vertices."""
    s, pool = len(degrees), max(degrees)
    edges = np.array([(i, s + j) for i, k in enumerate(degrees) for j in range(k)], dtype=np.int32).reshape(-1, 2)
    return cloud(s + pool, D), edges


def hub():
    """One hub joined to 5000 of 6000 vertices (79 pieces of 64 slots), the rest of the graph a sparse matching."""
    e = np.column_stack([np.zeros(5000), np.arange(1, 5001)])
    return cloud(6000, 2), np.concatenate([e, np.column_stack([np.arange(5001, 5999, 2), np.arange(5002, 6000, 2)])]).astype(np.int32)


def dims(D):
    return cloud(200, D), random_edges(200, 600)


def with_nan():
    pos, edges = cloud(120), random_edges(120, 500)
    pos[17, 1] = np.nan
    return pos, edges


def with_inf():
    pos, edges = cloud(120), random_edges(120, 500)
    pos[17, 1] = np.inf
    return pos, edges


def huge():
    """Coordinates of +-1e20: every square overflows, most distances are +inf and tie there."""
    pos, edges = cloud(120), random_edges(120, 500)
    return (np.sign(pos) * np.float32(1e20)).astype(np.float32), edges


def messy():
    """Self-loops, repeats and both directions."""
    e = random_edges(80, 300)
    e[::7, 1] = e[::7, 0]
    return cloud(80), np.concatenate([e, e[::3, ::-1], e[::5]])


CASES = {
    "n1": functools.partial(no_edges, 1), "n2": lambda: (cloud(2), np.array([[0, 1]], dtype=np.int32)),
    "no_edges": functools.partial(no_edges, 10), "isolated": lambda: (cloud(20), random_edges(20, 6)),
    "k5": functools.partial(complete, 5), "star": star, "path7": path7, "grid12": grid12, "clones": clones, "identical": identical,
    "ladder": functools.partial(ladder, list(range(13)) + [63, 64, 65, 300]), "pieces": functools.partial(ladder, [64, 65, 128, 129]),
    "hub": hub, "nan": with_nan, "inf": with_inf, "huge": huge, "messy": messy,
}
CASES.update({f"d{D}": functools.partial(dims, D) for D in DIMS})


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement's arrays for a case, computed once and shared by the CPU and the GPU tests (read-only)."""
    pos, edges = CASES[name]()
    out = ref.neighbor_ranks(pos, edges)
    for a in out.values():
        a.setflags(write=False)
    return pos, edges, out


def assert_same(got, want, what=""):
    assert list(got) == list(ARRAYS), what
    for key in ARRAYS:
        assert got[key].shape == want[key].shape, (what, key)
        same = ref.same_bits(got[key], want[key]) if key == "dist2" else np.array_equal(got[key], want[key])
        assert same, (what, key)
    assert got["neighbors"].dtype == np.int32 and got["dist2"].dtype == np.float32
    assert all(got[key].dtype == np.int64 for key in ("sources", "indptr", "below", "equal"))


def check_against_restatement(device_id, name):
    pos, edges, want = reference(name)
    assert_same(gr.neighbor_ranks(pos, edges, device_id=device_id), want, name)


def check_strided(device_id):
    """The same positions inside a wider buffer (ld > D)."""
    pos, edges, want = reference("d3")
    wide = np.full((len(pos), 7), np.float32(1e30))
    wide[:, :3] = pos
    q = _native.LayoutQuality(edges, len(pos), device_id)
    try:
        q.set_positions(wide, D=3, ld=7)
        indptr, neighbors, dist2, below, equal = q.neighbor_ranks()
        assert below.dtype == np.int32 and equal.dtype == np.int32
        assert np.array_equal(indptr, want["indptr"]) and np.array_equal(neighbors, want["neighbors"])
        assert ref.same_bits(dist2, want["dist2"]) and np.array_equal(below, want["below"]) and np.array_equal(equal, want["equal"])
    finally:
        q.close()


def check_rows(device_id, name="ladder"):
    """Empty, one id, repeats, shuffled: each result equals the matching slices of the all-rows result."""
    pos, edges, want = reference(name)
    n = len(pos)
    rng = np.random.default_rng(2)
    for rows in ([], [n - 1], [16, 16, 0, 16, n - 1, 0, 13], rng.permutation(n), np.r_[rng.integers(0, n, 50), rng.integers(0, 17, 20)]):
        rows = np.asarray(rows, dtype=np.int64)
        got = gr.neighbor_ranks(pos, edges, rows=rows, device_id=device_id)
        assert np.array_equal(got["sources"], rows)
        assert np.array_equal(np.diff(got["indptr"]), np.diff(want["indptr"])[rows])
        for key in ("neighbors", "dist2", "below", "equal"):
            pieces = [want[key][want["indptr"][u]:want["indptr"][u + 1]] for u in rows]
            expect = np.concatenate(pieces) if pieces else want[key][:0]
            assert ref.same_bits(got[key], expect) if key == "dist2" else np.array_equal(got[key], expect), key


# ---- host path == restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_host_path_equals_restatement(name):
    check_against_restatement(-1, name)


def test_path_on_a_line_by_hand():
    """0 - 1 - ... - 6 drawn at x = 0 .. 6.  Every neighbour is at squared distance 1.  An interior vertex has both its
    neighbours there and nothing nearer: below = 0, equal = 1 (the other neighbour).  An end has one neighbour, nothing
    nearer, nothing as near."""
    pos, edges = path7()
    got = gr.neighbor_ranks(pos, edges, device_id=-1)
    assert got["sources"].tolist() == [0, 1, 2, 3, 4, 5, 6]
    assert got["indptr"].tolist() == [0, 1, 3, 5, 7, 9, 11, 12]
    assert got["neighbors"].tolist() == [1, 0, 2, 1, 3, 2, 4, 3, 5, 4, 6, 5]
    assert got["dist2"].tolist() == [1.0] * 12
    assert got["below"].tolist() == [0] * 12
    assert got["equal"].tolist() == [0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0]
    assert gr.link_auc(pos, edges, device_id=-1) == 1.0
    assert gr.neighborhood_preservation(pos, edges, device_id=-1) == {"precision": 1.0, "jaccard": 1.0}


def test_degenerate_cases_by_hand():
    for name in ("n1", "no_edges"):
        pos, edges, _ = reference(name)
        got = gr.neighbor_ranks(pos, edges, device_id=-1)
        assert got["indptr"].tolist() == [0] * (len(pos) + 1) and all(len(got[k]) == 0 for k in ("neighbors", "dist2", "below", "equal"))
        assert math.isnan(gr.link_auc(pos, edges, device_id=-1))
    pos, edges, _ = reference("n2")
    got = gr.neighbor_ranks(pos, edges, device_id=-1)
    assert got["neighbors"].tolist() == [1, 0] and got["below"].tolist() == [0, 0] and got["equal"].tolist() == [0, 0]
    assert math.isnan(gr.link_auc(pos, edges, device_id=-1))            # m_u = 0 for both
    pos, edges, _ = reference("k5")
    got = gr.neighbor_ranks(pos, edges, device_id=-1)
    assert np.array_equal(np.diff(got["indptr"]), [4] * 5) and sorted(got["below"][:4].tolist()) == [0, 1, 2, 3]
    assert math.isnan(gr.link_auc(pos, edges, device_id=-1))            # no non-neighbour anywhere
    assert gr.neighborhood_preservation(pos, edges, device_id=-1) == {"precision": 1.0, "jaccard": 1.0}
    got = gr.neighbor_ranks(pos, edges, rows=[], device_id=-1)           # n_rows = 0
    assert got["indptr"].tolist() == [0] and len(got["sources"]) == 0 and len(got["below"]) == 0


def test_ties_are_there():
    """The tie cases do have ties, and the clones do have thresholds of zero."""
    assert reference("grid12")[2]["equal"].max() >= 3
    c = reference("clones")[2]
    assert (c["dist2"] == 0).any() and c["equal"][c["dist2"] == 0].min() >= 8   # nine clones besides u, v is one of them
    i = reference("identical")[2]
    assert (i["dist2"] == 0).all() and (i["below"] == 0).all() and (i["equal"] == 38).all()
    h = reference("huge")[2]
    assert np.isinf(h["dist2"]).any() and h["equal"][np.isinf(h["dist2"])].min() > 0
    nn = reference("nan")[2]
    assert np.isnan(nn["dist2"]).any() and (nn["equal"][np.isnan(nn["dist2"])] == 0).all() and (nn["below"][np.isnan(nn["dist2"])] == 0).all()


def test_ladder_has_its_degrees():
    _, _, want = reference("ladder")
    assert np.diff(want["indptr"])[:17].tolist() == list(range(13)) + [63, 64, 65, 300]
    _, _, want = reference("hub")
    assert np.diff(want["indptr"])[0] == 5000


def test_canonicalisation():
    """An edge list with self-loops, repeats and both directions gives the arrays of its simple graph."""
    pos, edges, want = reference("messy")
    gp, gi = ref.simple_graph(len(pos), edges)
    simple = np.column_stack([np.repeat(np.arange(len(pos)), np.diff(gp)), gi])
    simple = simple[simple[:, 0] < simple[:, 1]]
    assert len(simple) < len(edges) / 1.3
    assert_same(gr.neighbor_ranks(pos, simple, device_id=-1), want)
    adj = sp.csr_matrix((np.ones(len(edges)), (edges[:, 0], edges[:, 1])), shape=(len(pos),) * 2)
    assert_same(gr.neighbor_ranks(pos, adj + adj.T, device_id=-1), want)   # the adjacency form


def test_strided_positions():
    check_strided(-1)


def test_rows():
    check_rows(-1)


def test_second_call_and_crossings_share_the_handle():
    """The neighbour query neither disturbs the crossing functions of the same handle nor is disturbed by new positions."""
    pos, edges, want = reference("d3")
    q = _native.LayoutQuality(edges, len(pos), -1)
    q.set_positions(pos)
    before = q.crossings()
    first, again = q.neighbor_ranks(), q.neighbor_ranks()
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(first, again)) and np.array_equal(first[3], want["below"])
    assert np.array_equal(q.crossings()[0], before[0])
    q.set_positions(pos[::-1].copy())
    assert not np.array_equal(q.neighbor_ranks()[3], want["below"])
    q.close()


def test_errors():
    pos, edges, _ = reference("d3")
    n = len(pos)
    q = _native.LayoutQuality(edges, n, -1)
    with pytest.raises(ValueError, match="no positions were set"):
        q.neighbor_ranks()
    with pytest.raises(ValueError, match="no positions were set"):
        q.neighbor_ranks([0])
    q.set_positions(pos)
    for bad in ([n], [-1], [0, 3, n]):
        with pytest.raises(ValueError, match=rf"row {len(bad) - 1} has a vertex id outside \[0, n\)"):
            q.neighbor_ranks(bad)
    with pytest.raises(ValueError, match=r"row 0 has a vertex id outside \[0, n\)"):
        gr.link_auc(pos, edges, rows=[n], device_id=-1)
    q.close()
    with pytest.raises(ValueError, match="handle is NULL"):
        q.neighbor_ranks()
    with pytest.raises(ValueError, match="edges are needed"):
        gr.neighbor_ranks(pos)


# ---- the measures ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def er300():
    """Gaussian positions and Erdos-Renyi edges in the style of the golden case c1_er1000 (p = 0.01 there), n = 300."""
    rng = np.random.default_rng(42)
    i, j = np.triu_indices(300, 1)
    keep = rng.random(len(i)) < 0.03
    return cloud(300), np.column_stack([i[keep], j[keep]]).astype(np.int32)


def check_measures(device_id):
    pos, edges = er300()
    n = len(pos)
    for rows in (None, np.random.default_rng(1).permutation(n)[:40]):
        assert gr.link_auc(pos, edges, rows=rows, device_id=device_id) == ref.link_auc(pos, edges, rows)
        got = gr.neighborhood_preservation(pos, edges, rows=rows, device_id=device_id)
        precision, jaccard = ref.neighborhood_preservation(pos, edges, rows)
        assert got["precision"] == precision
        assert abs(got["jaccard"] - jaccard) <= n * 2.0 ** -53 * jaccard
    assert 0.3 < gr.link_auc(pos, edges, device_id=device_id) < 0.7     # unrelated positions: no better than chance


def test_measures_equal_brute_force():
    check_measures(-1)


def test_measures_on_ties_equal_brute_force():
    """On the lattice and on clones the halves for ties and the ties in the neighbour's favour are in play."""
    for name in ("grid12", "clones", "ladder"):
        pos, edges, _ = reference(name)
        assert gr.link_auc(pos, edges, device_id=-1) == ref.link_auc(pos, edges), name
        got = gr.neighborhood_preservation(pos, edges, device_id=-1)
        precision, jaccard = ref.neighborhood_preservation(pos, edges)
        assert got["precision"] == precision and abs(got["jaccard"] - jaccard) <= len(pos) * 2.0 ** -53 * jaccard, name


def planted():
    """Two tight clusters far apart, each a clique: every neighbour is nearer than every non-neighbour."""
    pos = cloud(40) * np.float32(0.01)
    pos[20:, 0] += np.float32(100)
    i, j = np.triu_indices(20, 1)
    return pos, np.concatenate([np.column_stack([i, j]), np.column_stack([i + 20, j + 20])]).astype(np.int32)


def test_planted_layout_is_perfect():
    pos, edges = planted()
    assert gr.link_auc(pos, edges, device_id=-1) == 1.0
    assert gr.neighborhood_preservation(pos, edges, device_id=-1) == {"precision": 1.0, "jaccard": 1.0}
    out = gr.embedding_quality(pos, edges, device_id=-1)
    assert out["link_auc"] == 1.0 and out["neighborhood_precision"] == 1.0 and out["mean_rank"] == 0.0


def test_embedding_quality_keys_and_sampling():
    pos, edges = er300()
    n = len(pos)
    out = gr.embedding_quality(pos, edges, device_id=-1)
    assert list(out) == ["n_vertices", "sources", "sources_exact", "link_auc", "neighborhood_precision", "neighborhood_jaccard", "mean_rank"]
    assert out["n_vertices"] == n and out["sources"] == n and out["sources_exact"] is True
    assert out["link_auc"] == ref.link_auc(pos, edges)
    assert out["neighborhood_precision"] == ref.neighborhood_preservation(pos, edges)[0]
    want = ref.neighbor_ranks(pos, edges)
    b_bar = sum(int(want["below"][s]) - int(np.count_nonzero(want["dist2"][lo:hi] < want["dist2"][s]))
                for lo, hi in zip(want["indptr"][:-1], want["indptr"][1:]) for s in range(lo, hi))
    assert out["mean_rank"] == b_bar / len(want["below"])
    # sampled: rows = sort(default_rng(seed).choice(n, S, replace=False))
    est = gr.embedding_quality(pos, edges, exact=False, sample_size=50, seed=3, device_id=-1)
    rows = np.sort(np.random.default_rng(3).choice(n, 50, replace=False))
    assert est["sources"] == 50 and est["sources_exact"] is False
    assert est["link_auc"] == ref.link_auc(pos, edges, rows) == gr.link_auc(pos, edges, rows=rows, device_id=-1)
    assert est["neighborhood_precision"] == ref.neighborhood_preservation(pos, edges, rows)[0]
    # a sample of every vertex is exact; exact=True ignores the sample size; exact=None goes by the threshold
    assert gr.embedding_quality(pos, edges, exact=False, sample_size=n, device_id=-1) == out
    assert gr.embedding_quality(pos, edges, exact=True, sample_size=5, device_id=-1) == out
    assert quality.HOST_EXACT_MAX_VERTICES >= n and quality.EXACT_MAX_VERTICES >= quality.HOST_EXACT_MAX_VERTICES
    old = quality.HOST_EXACT_MAX_VERTICES
    try:
        quality.HOST_EXACT_MAX_VERTICES = n - 1
        assert gr.embedding_quality(pos, edges, sample_size=50, seed=3, device_id=-1) == est
    finally:
        quality.HOST_EXACT_MAX_VERTICES = old
    empty = gr.embedding_quality(np.zeros((3, 2)), np.zeros((0, 2), dtype=np.int32), device_id=-1)
    assert empty["sources"] == 3 and math.isnan(empty["link_auc"]) and math.isnan(empty["neighborhood_precision"]) and math.isnan(empty["mean_rank"])


def test_layout_quality_is_unchanged():
    pos, edges = er300()
    assert list(gr.layout_quality(pos, edges, device_id=-1)) == ["n_edges", "crossings", "crossings_stderr", "crossings_exact",
                                                                "crossings_per_edge", "min", "max", "mean", "std"]


def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "graphem_hip.h")).read()
    lib = _native.load()
    for name in RANK_SYMBOLS:
        assert name + "(" in header and name in _native.SYMBOLS and hasattr(lib, name), name
    for name in ("neighbor_ranks", "link_auc", "neighborhood_preservation", "embedding_quality"):
        assert name in gr.__all__ and hasattr(gr, name), name
    assert callable(gr.GraphEmbedderHIP.embedding_quality)
