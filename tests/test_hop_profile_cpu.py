"""The hop profile and the distance-preservation measures without a GPU (csrc/quality.hip host path, graphem-rapids_amd/
quality.py) against the restatement of the header's rule (tests/hops_reference.py).

The comparison rule, used everywhere: integers and the bits of min_d2 / max_d2 must be EQUAL; a double sum of N
non-negative terms is held to (N + 8) 2^-52 relative against the reference and is exactly 0 when N = 0.  That bound is
derived, not measured: any order of summation of N non-negative doubles is within (N - 1) 2^-53 of the true sum, and a
term carries at most three roundings (the square root, the division, the product of a partial sum by 1 / h).

The derived measures (stress, scale, vertex stress, Pearson's r, the standard error) are checked the second way the rule
allows: the library's own formula (quality._stress, quality._hop_correlation; the standard error is restated here) is
applied to the REFERENCE sums and the library's result must agree at 1e-12 relative; the layouts of those tests are far
from a zero stress and a zero correlation, where the quotients would cancel."""
import functools
import math
import os

import numpy as np
import pytest

import graphem_rapids_amd as gr
from graphem_rapids_amd import _native, quality
import graphstats_reference as gsref
import hops_reference as href
import neighbors_reference as nref

HOP_SYMBOLS = ["gh_qual_hop_profile"]
PUBLIC = ["hop_profile", "layout_stress", "hop_distance_correlation", "distance_quality"]
INTS = ("sources", "hops", "pairs", "reach", "eccentricity")
KEYS = ("sources", "hops", "pairs", "sum_d", "sum_d2", "min_d2", "max_d2", "mean_d", "reach", "eccentricity", "sum_d_over_h",
        "sum_d2_over_h2", "n_unreachable")
DIMS = [1, 2, 3, 16, 130]   # 130: 64 source rows of 130 floats do not fit the kernel's LDS, so they are read from memory


# ---- the inputs ------------------------------------------------------------------------------------------------------
def _edges(pairs):
    return np.asarray(pairs, dtype=np.int64).reshape(-1, 2)


def grid(rows=7, cols=9):
    ids = np.arange(rows * cols).reshape(rows, cols)
    return _edges(np.concatenate([np.column_stack([ids[:, :-1].ravel(), ids[:, 1:].ravel()]),
                                  np.column_stack([ids[:-1].ravel(), ids[1:].ravel()])]))


GRAPHS = {
    "n1": lambda: (1, _edges([])),
    "n2": lambda: (2, _edges([[0, 1]])),
    "no_edges": lambda: (5, _edges([])),
    "components": lambda: (9, _edges([[0, 1], [1, 2], [2, 3], [4, 5], [5, 6], [6, 4], [6, 7]])),   # a path, a triangle with a tail, 8 alone
    "k5": lambda: (5, _edges(np.column_stack(np.triu_indices(5, 1)))),
    "star": lambda: (41, _edges(np.column_stack([np.zeros(40), np.arange(1, 41)]))),
    "cycle": lambda: (17, _edges(np.column_stack([np.arange(17), (np.arange(17) + 1) % 17]))),
    "grid": lambda: (63, grid()),
    "path130": lambda: (130, gsref.permuted_path(130)),   # hops up to 129: more than 64 levels, across the flag-poll boundary
    "regular": lambda: (300, gsref.messy(300, gr.random_regular_edges(300, 3, seed=1))),   # duplicates, self-loops, both directions
}


def cloud(n, D, seed=0):
    return np.random.default_rng(700 + n + 31 * D + seed).standard_normal((n, D)).astype(np.float32)


def coincident(n, D=3):
    """n vertices on 4 positions: d2 = 0 between the clones."""
    return cloud(4, D)[np.arange(n) % 4]


def source_lists(n):
    """None, none, a repeat, and 130 random ids: groups of 64 + 64 + 2."""
    lists = {"all": None, "empty": np.zeros(0, dtype=np.int64), "random": np.random.default_rng(n).integers(0, n, 130)}
    if n >= 4:
        lists["repeat"] = np.array([3, 3, 0])
    return lists


@functools.lru_cache(maxsize=None)
def graph(name):
    """(n, edges, the matrix of hop distances) of a graph, computed once and shared (read-only)."""
    n, edges = GRAPHS[name]()
    hops = href.all_hops(n, edges)
    hops.setflags(write=False)
    edges.setflags(write=False)
    return n, edges, hops


@functools.lru_cache(maxsize=None)
def reference(name, D, layout="cloud"):
    """pos and the restatement's profile per source list for one (graph, D, layout), computed once and shared by the CPU
    and the GPU tests (read-only)."""
    n, edges, hops = graph(name)
    pos = cloud(n, D) if layout == "cloud" else coincident(n, D)
    want = {key: href.hop_profile(pos, edges, src, hops) for key, src in source_lists(n).items()}
    for w in want.values():
        for a in w.values():
            a.setflags(write=False)
    return pos, want


CASES = [(name, D) for name in GRAPHS for D in DIMS]


# ---- the comparison rule ----------------------------------------------------------------------------------------------
def assert_profile(got, want, n, what=""):
    """got: hop_profile's dict; want: the restatement's."""
    assert tuple(got) == KEYS, what
    H = len(want["pairs"])
    assert np.array_equal(got["hops"], np.arange(1, H + 1)) and got["hops"].dtype == np.int64, what
    for key in ("sources", "pairs", "reach", "eccentricity"):
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (what, key)
    for key in ("min_d2", "max_d2"):
        assert got[key].dtype == np.float32 and nref.same_bits(got[key], want[key]), (what, key)
    for key, terms in (("sum_d", "pairs"), ("sum_d2", "pairs"), ("sum_d_over_h", "reach"), ("sum_d2_over_h2", "reach")):
        assert got[key].dtype == np.float64 and href.close(got[key], want[key], want[terms]), (what, key)
    assert np.array_equal(got["mean_d"], got["sum_d"] / got["pairs"]), what
    assert got["n_unreachable"] == len(want["sources"]) * (n - 1) - int(want["reach"].sum()), what


def same_exact_part(a, b):
    """Two results of the library: integers and min / max bits equal."""
    return (all(np.array_equal(a[key], b[key]) for key in INTS) and a["n_unreachable"] == b["n_unreachable"]
            and nref.same_bits(a["min_d2"], b["min_d2"]) and nref.same_bits(a["max_d2"], b["max_d2"]))


def assert_agree(a, b, what=""):
    """Two results of the library, by whichever paths: the exact part equal, each sum within the rule of the other."""
    assert same_exact_part(a, b), what
    for key, terms in (("sum_d", "pairs"), ("sum_d2", "pairs"), ("sum_d_over_h", "reach"), ("sum_d2_over_h2", "reach")):
        # each is within (N + 2) 2^-53 of the true sum (the header), so they are within the rule's (N + 8) 2^-52 of each other
        assert href.close(a[key], b[key], a[terms]), (what, key)


def check_case(device_id, name, D):
    """One (graph, D) under every source list."""
    n, edges, _ = graph(name)
    pos, want = reference(name, D)
    for key, src in source_lists(n).items():
        assert_profile(gr.hop_profile(pos, edges, sources=src, device_id=device_id), want[key], n, (name, D, key))


def check_coincident(device_id, name):
    n, edges, _ = graph(name)
    pos, want = reference(name, 3, "coincident")
    for key, src in source_lists(n).items():
        assert_profile(gr.hop_profile(pos, edges, sources=src, device_id=device_id), want[key], n, (name, key))
    if name in ("star", "cycle", "grid", "path130", "regular"):   # connected and more than 4 vertices: two clones are a pair
        assert want["all"]["min_d2"].min() == 0.0


def check_strided(device_id, name="regular"):
    """The same positions inside a wider buffer (ld > D)."""
    n, edges, _ = graph(name)
    pos, want = reference(name, 3)
    wide = np.full((n, 7), np.float32(1e30))
    wide[:, :3] = pos
    q = _native.LayoutQuality(edges, n, device_id)
    try:
        q.set_positions(wide, D=3, ld=7)
        for key, src in source_lists(n).items():
            got, w = q.hop_profile(src), want[key]
            assert np.array_equal(got["pairs"], w["pairs"]) and np.array_equal(got["reach"], w["reach"])
            assert np.array_equal(got["eccentricity"], w["eccentricity"]) and got["eccentricity"].dtype == np.int32
            assert nref.same_bits(got["min_d2"], w["min_d2"]) and nref.same_bits(got["max_d2"], w["max_d2"])
            assert href.close(got["sum_d"], w["sum_d"], w["pairs"]) and href.close(got["sum_d2_over_h2"], w["sum_d2_over_h2"], w["reach"])
    finally:
        q.close()


def check_non_finite(device_id):
    """A NaN row and an infinite row: the integers stay exact."""
    n, edges, _ = graph("grid")
    pos, want = reference("grid", 3)
    bad = pos.copy()
    bad[5, 1], bad[40, 0] = np.nan, np.inf
    with np.errstate(all="ignore"):
        got = gr.hop_profile(bad, edges, device_id=device_id)
    for key in ("pairs", "reach", "eccentricity"):
        assert np.array_equal(got[key], want["all"][key]), key


def rel(a, b, tol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((np.abs(a - b) <= tol * np.abs(b)) | (np.isnan(a) & np.isnan(b))))


def noisy_lattice():
    """The 7 x 9 grid near its lattice: a stress well above 0 and a correlation well below 1, neither near a cancellation."""
    i = np.arange(63)
    return (np.column_stack([i % 9, i // 9, np.zeros(63)]) + 0.3 * cloud(63, 3)).astype(np.float32)


def as_profile(want, n):
    """The restatement's sums in the shape quality._stress and quality._hop_correlation take."""
    out = dict(want)
    out["hops"] = np.arange(1, len(want["pairs"]) + 1, dtype=np.int64)
    out["n_unreachable"] = len(want["sources"]) * (n - 1) - int(want["reach"].sum())
    return out


def stderr_from(want, n, S):
    """The ratio estimator's error from the reference sums, restated."""
    a, b, c = want["sum_d_over_h"], want["sum_d2_over_h2"], want["reach"]
    s = math.fsum(a) / math.fsum(b)
    t = s * s * b - 2 * s * a + c
    stress = math.fsum(t) / int(c.sum())
    return math.sqrt(S / (S - 1) * math.fsum((t - stress * c) ** 2)) / int(c.sum()) * math.sqrt(1 - S / n)


def check_measures(device_id):
    n, edges, hops = graph("grid")
    pos = noisy_lattice()
    want = as_profile(href.hop_profile(pos, edges, None, hops), n)
    for scale in (None, 0.7):
        got, ref = gr.layout_stress(pos, edges, scale=scale, device_id=device_id), quality._stress(want, scale)[0]   # pylint: disable=protected-access
        assert list(got) == ["stress", "scale", "pairs", "n_unreachable", "sources", "vertex_stress"]
        assert got["pairs"] == ref["pairs"] == 63 * 62 and got["n_unreachable"] == 0 and np.array_equal(got["sources"], np.arange(63))
        assert rel(got["stress"], ref["stress"]) and rel(got["scale"], ref["scale"]) and rel(got["vertex_stress"], ref["vertex_stress"])
        assert 0.005 < got["stress"] < 1
    assert gr.layout_stress(pos, edges, scale=0.7, device_id=device_id)["scale"] == 0.7
    r = gr.hop_distance_correlation(pos, edges, device_id=device_id)
    assert rel(r, quality._hop_correlation(want)) and 0.5 < r < 0.999   # pylint: disable=protected-access
    # positions times 2^-3: every d2 is scaled exactly, so the stress stays and the scale takes the factor
    base, small = gr.layout_stress(pos, edges, device_id=device_id), gr.layout_stress(pos * np.float32(0.125), edges, device_id=device_id)
    assert rel(small["stress"], base["stress"]) and rel(small["scale"], 8 * base["scale"])
    # a subset of sources, and a source that reaches nothing
    n, edges, hops = graph("components")
    pos, _ = reference("components", 3)
    src = [8, 0, 5, 8]
    want = as_profile(href.hop_profile(pos, edges, src, hops), n)
    got, ref = gr.layout_stress(pos, edges, sources=src, device_id=device_id), quality._stress(want)[0]   # pylint: disable=protected-access
    assert np.isnan(got["vertex_stress"][[0, 3]]).all() and rel(got["vertex_stress"], ref["vertex_stress"]) and rel(got["stress"], ref["stress"])
    assert got["pairs"] == 3 + 3 and got["n_unreachable"] == 4 * 8 - 6
    assert gr.hop_profile(pos, edges, device_id=device_id)["n_unreachable"] == 9 * 8 - (4 * 3 + 4 * 3)
    empty = gr.layout_stress(pos, edges, sources=[8], device_id=device_id)
    assert math.isnan(empty["stress"]) and empty["scale"] == 1.0 and empty["pairs"] == 0
    assert math.isnan(gr.hop_distance_correlation(pos, edges, sources=[8], device_id=device_id))


def check_distance_quality(device_id):
    n, edges, hops = graph("regular")
    pos, want = reference("regular", 3)
    out = gr.distance_quality(pos, edges, device_id=device_id)
    assert list(out) == ["n_sources", "exact", "pairs", "n_unreachable", "stress", "scale", "stress_stderr", "correlation", "hops",
                         "mean_d", "max_hop"]
    ref = quality._stress(as_profile(want["all"], n))[0]   # pylint: disable=protected-access
    assert out["n_sources"] == n and out["exact"] is True and out["stress_stderr"] == 0.0 and out["pairs"] == int(want["all"]["reach"].sum())
    assert rel(out["stress"], ref["stress"]) and rel(out["scale"], ref["scale"]) and out["max_hop"] == len(want["all"]["pairs"])
    assert np.array_equal(out["hops"], np.arange(1, out["max_hop"] + 1)) and href.close(out["mean_d"] * want["all"]["pairs"], want["all"]["sum_d"], want["all"]["pairs"] + 1)
    for S in (n, n + 5):   # S >= n: every vertex
        full = gr.distance_quality(pos, edges, exact=False, sample_size=S, device_id=device_id)
        assert full["exact"] is True and full["stress_stderr"] == 0.0 and full["pairs"] == out["pairs"]
    est = gr.distance_quality(pos, edges, exact=False, sample_size=50, seed=3, device_id=device_id)
    src = np.sort(np.random.default_rng(3).choice(n, 50, replace=False))
    sampled = href.hop_profile(pos, edges, src, hops)
    ref = quality._stress(as_profile(sampled, n))[0]   # pylint: disable=protected-access
    assert est["n_sources"] == 50 and est["exact"] is False and est["pairs"] == int(sampled["reach"].sum())
    assert rel(est["stress"], ref["stress"]) and rel(est["stress_stderr"], stderr_from(sampled, n, 50)) and est["stress_stderr"] > 0
    assert abs(est["stress"] - out["stress"]) < 6 * est["stress_stderr"]
    again = gr.distance_quality(pos, edges, exact=False, sample_size=50, seed=3, device_id=device_id)
    other = gr.distance_quality(pos, edges, exact=False, sample_size=50, seed=4, device_id=device_id)
    assert again["pairs"] == est["pairs"] and rel(again["stress"], est["stress"]) and other["stress"] != est["stress"]
    one = gr.distance_quality(pos, edges, exact=False, sample_size=1, device_id=device_id)
    assert one["n_sources"] == 1 and one["stress_stderr"] == 0.0


# ---- the tests -------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "graphem_hip.h")).read()
    lib = _native.load()
    for name in HOP_SYMBOLS:
        assert name + "(" in header and name in _native.SYMBOLS and name in _native.SIGNATURES and hasattr(lib, name), name
    assert "distance preservation" in header
    for name in PUBLIC:
        assert name in gr.__all__ and getattr(gr, name) is getattr(quality, name), name
    assert callable(_native.LayoutQuality.hop_profile)


def test_path_of_33_is_exact():
    n = 33
    pos = np.column_stack([np.arange(n), np.zeros(n)]).astype(np.float32)
    edges = np.column_stack([np.arange(n - 1), np.arange(1, n)])
    p = gr.hop_profile(pos, edges, device_id=-1)
    h = np.arange(1, n)
    assert np.array_equal(p["hops"], h) and np.array_equal(p["pairs"], 2 * (n - h))
    assert np.array_equal(p["sum_d"], 2.0 * h * (n - h)) and np.array_equal(p["sum_d2"], 2.0 * h * h * (n - h))
    assert np.array_equal(p["min_d2"], (h * h).astype(np.float32)) and np.array_equal(p["max_d2"], p["min_d2"])
    assert np.array_equal(p["reach"], np.full(n, n - 1)) and np.array_equal(p["eccentricity"], np.maximum(np.arange(n), n - 1 - np.arange(n)))
    assert np.array_equal(p["mean_d"], h.astype(np.float64)) and p["n_unreachable"] == 0
    s = gr.layout_stress(pos, edges, device_id=-1)
    assert s["stress"] == 0.0 and s["scale"] == 1.0 and s["pairs"] == n * (n - 1) and np.array_equal(s["vertex_stress"], np.zeros(n))
    assert abs(gr.hop_distance_correlation(pos, edges, device_id=-1) - 1.0) <= 1e-12
    s4 = gr.layout_stress(pos * 4, edges, device_id=-1)
    assert s4["scale"] == 0.25 and s4["stress"] == 0.0
    q = gr.distance_quality(pos, edges, device_id=-1)
    assert q["stress"] == 0.0 and q["scale"] == 1.0 and q["max_hop"] == n - 1 and q["exact"] is True


@pytest.mark.parametrize("name,D", CASES)
def test_host_path_equals_restatement(name, D):
    check_case(-1, name, D)


@pytest.mark.parametrize("name", list(GRAPHS))
def test_coincident_points(name):
    check_coincident(-1, name)


def test_strided_positions():
    check_strided(-1)


def test_non_finite_rows_leave_the_integers_exact():
    check_non_finite(-1)


def test_edge_order_duplicates_and_thread_count_do_not_matter():
    """The messy edge list against the clean one, and sources in another order: the exact part is equal."""
    n, edges, _ = graph("regular")
    pos, _ = reference("regular", 3)
    clean = gr.random_regular_edges(300, 3, seed=1)
    a, b = gr.hop_profile(pos, edges, device_id=-1), gr.hop_profile(pos, clean, device_id=-1)
    assert_agree(a, b)
    src = np.random.default_rng(8).permutation(n)
    c = gr.hop_profile(pos, edges, sources=src, device_id=-1)
    assert np.array_equal(c["pairs"], a["pairs"]) and nref.same_bits(c["min_d2"], a["min_d2"]) and nref.same_bits(c["max_d2"], a["max_d2"])
    assert np.array_equal(c["reach"], a["reach"][src]) and np.array_equal(c["eccentricity"], a["eccentricity"][src])


def test_measures():
    check_measures(-1)


def test_distance_quality():
    check_distance_quality(-1)


def test_exact_none_follows_the_host_constant(monkeypatch):
    n, edges, _ = graph("grid")
    pos, _ = reference("grid", 3)
    assert gr.distance_quality(pos, edges, sample_size=10, device_id=-1)["exact"] is True
    monkeypatch.setattr(quality, "HOST_EXACT_MAX_DISTANCE_VERTICES", 62)
    out = gr.distance_quality(pos, edges, sample_size=10, device_id=-1)
    assert out["exact"] is False and out["n_sources"] == 10
    assert quality.EXACT_MAX_DISTANCE_VERTICES >= quality.HOST_EXACT_MAX_DISTANCE_VERTICES > 0


def test_errors():
    n, edges, _ = graph("grid")
    pos, _ = reference("grid", 3)
    q = _native.LayoutQuality(edges, n, -1)
    with pytest.raises(ValueError, match="no positions were set"):
        q.hop_profile()
    with pytest.raises(ValueError, match="no positions were set"):
        q.hop_profile([0])
    q.set_positions(pos)
    for bad in ([n], [-1], [0, 3, n]):
        with pytest.raises(ValueError, match=rf"source {len(bad) - 1} has a vertex id outside \[0, n\)"):
            q.hop_profile(bad)
    with pytest.raises(ValueError, match=r"source 0 has a vertex id outside \[0, n\)"):
        gr.layout_stress(pos, edges, sources=[n], device_id=-1)
    q.close()
    with pytest.raises(ValueError, match="handle is NULL"):
        q.hop_profile()
    with pytest.raises(ValueError, match="edges are needed"):
        gr.hop_profile(pos)

    class Embedder:
        _engine = object()

    for fn in (gr.hop_profile, gr.layout_stress, gr.hop_distance_correlation, gr.distance_quality):
        with pytest.raises(ValueError, match="an embedder brings its own edges"):
            fn(Embedder(), edges)


def test_host_path_holds_no_device_allocation():
    n, edges, _ = graph("regular")
    pos, _ = reference("regular", 3)
    start = _native.live_allocations()
    q = _native.LayoutQuality(edges, n, -1)
    q.set_positions(pos)
    first, again = q.hop_profile(), q.hop_profile([5, 7])
    assert len(first["reach"]) == n and len(again["reach"]) == 2
    assert _native.live_allocations() == start
    q.close()
    assert _native.live_allocations() == start
