"""Layout quality on the GPU: exact edge-crossing counts and edge-length statistics of a layout.

The engine exists to push crossing edges apart; this module says how many pairs of edges of a layout do cross.  The count
is an integer defined by the engine's own test (include/graphem_hip.h "layout quality"): two edges without a common
vertex cross when, on coordinates 0 and 1, each one's endpoints lie strictly on opposite sides of the other in float32
arithmetic.  It is a float32 rule -- a float64 embedder's positions are rounded to float32 first -- and every pair of
edges is tested (csrc/quality.hip: an all-pairs HIP kernel; the host path of the library without a device).

Every function takes either a GraphEmbedderHIP, whose edges and device positions are used as they are (no download), or
(positions, edges): positions (n, D) array-like, edges an (E, 2) array or a scipy sparse adjacency.  An adjacency goes
through the embedder's own rule (upper triangle of the nonzero pattern in CSR row order), so edge ids equal the
embedder's.  Edge ids are kept as given: nothing is merged or dropped.

Embedding quality asks the other question: are a vertex's neighbours nearer to it than the vertices it is not joined to?
neighbor_ranks returns, for every (source, neighbour), how many other vertices lie strictly nearer and how many exactly
as near -- exact integers under the float32 distance of include/graphem_hip.h "embedding quality", over ALL D coordinates
and on the SIMPLE graph of the edge list (self-loops dropped, repeats and both directions merged) -- and link_auc,
neighborhood_preservation and embedding_quality are a few divisions of sums of those integers.

Distance preservation asks about the layout as a whole: does embedding distance follow graph distance?  hop_profile returns,
per hop and per source, the sums of the embedding distance over every (source, vertex) pair the graph joins (include/
graphem_hip.h "distance preservation": a breadth-first search from 64 sources to a machine word that evaluates the pair's
distance where the source first reaches the vertex), and layout_stress, hop_distance_correlation and distance_quality --
Kamada-Kawai stress, the Shepard curve, Pearson's r between hops and distance -- are a few operations on those sums.
"""
import math

import numpy as np
import scipy.sparse as sp

from . import _native

# layout_quality(exact=None) counts exactly up to this many edges and estimates above it.  Measured on one MI355X
# (2026-10-18, tools/layout_quality.py --n 100000 --iters 20 --time): the exact count of 400 000 edges
# takes 0.098 s, 1.63e12 pair tests per second, and the time grows with the square of E: 0.61 s at a million edges, a second
# at 1.28 million.  The estimate from 4096 sampled edges takes 1.2 ms at 400 000 edges.
EXACT_MAX_EDGES = 1_000_000
# The same for the library's host path (no device): 8.5 s at 400 000 edges on 16 threads of the same machine's host,
# 1.9e10 pair tests per second, a second at 137 000 edges.
HOST_EXACT_MAX_EDGES = 100_000
# embedding_quality(exact=None) takes every vertex as a source up to this many vertices and samples sources above it.
# Measured on one MI355X (2026-10-19, tools/embedding_quality.py --n 100000 --iters 20 --time --host and --n 1000000
# --iters 20 --time --host --repeats 2; random-regular d = 8, D = 3, the layout after 20 iterations):
# neighbor_ranks over all sources takes 0.0345 s at 100 K vertices and 3.19 s at a million, 2.9e11 and 3.1e11 (source,
# column) pairs per second, and the time grows with the square of n; the whole embedding_quality(exact=True) call takes
# 0.086 s and 3.61 s, so about 0.42 us per vertex on top of the kernel (graph, slots, numpy).  3.19e-12 n^2 + 0.42e-6 n is
# a second at 500 000 vertices.  4096 sampled sources take 1.6 ms at 100 K and 14.7 ms at a million.
EXACT_MAX_VERTICES = 500_000
# The same for the library's host path (no device): 4096 sources take 0.097 s at 100 K and 0.884 s at a million on 16
# threads of the same machine's host, 4.2e9 and 4.6e9 pairs per second; all sources were not run there, and at that rate
# they take a second at 66 000 vertices.
HOST_EXACT_MAX_VERTICES = 60_000
# distance_quality(exact=None) takes every vertex as a source up to this many vertices and samples sources above it.
# Measured on one MI355X (2026-10-19, tools/distance_quality.py --n 100000 --iters 20 --time --host --all and --n 1000000
# --iters 20 --time --host; random-regular d = 8, D = 3, the layout after 20 iterations, 8 and 9 hops):
# the hop profile over all sources takes 0.159 s at 100 K vertices, 6.3e10 (source, vertex) pairs per second, and the time
# grows with the square of n: 1.59e-11 n^2 is a second at 250 000 vertices (all sources were not run above 100 K).  1024
# sampled sources take 2.33 ms at 100 K and 20.8 ms at a million, 4.4e10 and 4.9e10 pairs per second; the whole
# distance_quality call on them takes 14 ms and 99 ms (graph, upload, numpy).
EXACT_MAX_DISTANCE_VERTICES = 250_000
# The same for the library's host path (no device): 1024 sources take 0.141 s at 100 K and 11.1 s at a million on 16
# threads of the same machine's host, 7.3e8 and 9.2e7 pairs per second (a search's distance array leaves the caches); all
# sources were not run there, and at the 100 K rate they take a second at 27 000 vertices.
HOST_EXACT_MAX_DISTANCE_VERTICES = 25_000


def _edges_from_adjacency(adjacency):
    """GraphEmbedderHIP._extract_edges_from_adjacency's rule: upper triangle of the nonzero pattern, CSR row order."""
    rows, cols = sp.csr_matrix(adjacency).nonzero()
    keep = rows < cols
    return np.column_stack([rows[keep], cols[keep]])


def _default_device():
    try:
        return 0 if _native.device_count() > 0 else -1
    except Exception:  # pylint: disable=broad-exception-caught
        return -1


class _Snapshot:
    """A LayoutQuality handle holding the layout of `x`: with-statement owner of the native handle."""

    def __init__(self, x, edges=None, device_id=None):
        engine = getattr(x, "_engine", None)
        if engine is not None:
            if edges is not None:
                raise ValueError("an embedder brings its own edges")
            self.L_min = float(x.L_min)
            self.q = _native.LayoutQuality(x._edges_np, x.n, x.device.index)   # pylint: disable=protected-access
            try:
                if engine.f64:
                    self.q.set_positions(engine.get_positions().astype(np.float32))   # the rule is a float32 rule
                else:
                    self.q.set_positions_device(engine.positions_unpadded_device_ptr(), engine.D)
            except Exception:
                self.q.close()
                raise
            return
        if edges is None:
            raise ValueError("edges are needed with positions")
        self.L_min = None
        pos = np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x)
        if pos.ndim != 2:
            raise ValueError(f"positions must be (n, D), got shape {pos.shape}")
        if sp.issparse(edges):
            if edges.shape[0] != pos.shape[0]:
                raise ValueError(f"adjacency of {edges.shape[0]} vertices with {pos.shape[0]} positions")
            edges = _edges_from_adjacency(edges)
        edges = np.asarray(edges).reshape(-1, 2)
        self.q = _native.LayoutQuality(edges, pos.shape[0], _default_device() if device_id is None else device_id)
        try:
            self.q.set_positions(pos.astype(np.float32))
        except Exception:
            self.q.close()
            raise

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.q.close()

    def estimate(self, sample_size, seed):
        E = self.q.E
        S = min(int(sample_size), E)
        if S < 1:
            return 0.0, 0.0
        rows = np.sort(np.random.default_rng(seed).choice(E, S, replace=False))
        counts, total = self.q.crossings(rows)
        if S == E:
            return total / 2, 0.0   # every row: the exact total
        estimate = E / (2 * S) * total
        stderr = E / 2 * np.std(counts.astype(np.float64), ddof=1) / np.sqrt(S) * np.sqrt(1 - S / E) if S >= 2 else 0.0
        return float(estimate), float(stderr)

    def ranks(self, rows=None):
        """neighbor_ranks' dict for the source ids `rows` (None: all vertices)."""
        indptr, neighbors, dist2, below, equal = self.q.neighbor_ranks(rows)
        sources = np.arange(self.q.n, dtype=np.int64) if rows is None else np.array(rows, dtype=np.int64).ravel()
        return {"sources": sources, "indptr": indptr, "neighbors": neighbors, "dist2": dist2,
                "below": below.astype(np.int64), "equal": equal.astype(np.int64)}

    def sample(self, exact, sample_size, seed):
        """The source ids embedding_quality uses: None (all vertices) or the sorted sample."""
        n = self.q.n
        if exact is None:
            exact = n <= (EXACT_MAX_VERTICES if self.q.device_id >= 0 else HOST_EXACT_MAX_VERTICES)
        S = min(int(sample_size), n)
        if exact or S >= n:
            return None
        return np.sort(np.random.default_rng(seed).choice(n, S, replace=False))

    def hops(self, sources=None):
        """hop_profile's dict for the source ids `sources` (None: all vertices)."""
        n = self.q.n
        p = self.q.hop_profile(sources)
        ids = np.arange(n, dtype=np.int64) if sources is None else np.array(sources, dtype=np.int64).ravel()
        mean_d = p["sum_d"] / p["pairs"]   # every hop up to H has a pair
        return {"sources": ids, "hops": np.arange(1, len(p["pairs"]) + 1, dtype=np.int64), "pairs": p["pairs"],
                "sum_d": p["sum_d"], "sum_d2": p["sum_d2"], "min_d2": p["min_d2"], "max_d2": p["max_d2"], "mean_d": mean_d,
                "reach": p["reach"], "eccentricity": p["eccentricity"], "sum_d_over_h": p["sum_d_over_h"],
                "sum_d2_over_h2": p["sum_d2_over_h2"], "n_unreachable": len(ids) * (n - 1) - int(p["reach"].sum())}

    def distance_sample(self, exact, sample_size, seed):
        """The source ids distance_quality uses: None (all vertices) or the sorted sample."""
        n = self.q.n
        if exact is None:
            exact = n <= (EXACT_MAX_DISTANCE_VERTICES if self.q.device_id >= 0 else HOST_EXACT_MAX_DISTANCE_VERTICES)
        S = min(int(sample_size), n)
        if exact or S >= n:
            return None
        return np.sort(np.random.default_rng(seed).choice(n, S, replace=False))

    def length_stats(self):
        E = self.q.E
        mn, mx, s, ss = (float(v) for v in self.q.edge_lengths())
        if E == 0:
            return {"min": mn, "max": mx, "mean": float("nan"), "std": float("nan")}
        mean = s / E
        return {"min": mn, "max": mx, "mean": mean, "std": float(np.sqrt(max(ss / E - mean * mean, 0.0)))}


def edge_crossing_counts(x, edges=None, rows=None, device_id=None):
    """int64 array: for every edge id in `rows` (any order, repeats allowed; None = all edges in order) the number of
    edges that cross it.  With all edges the layout's crossing number is counts.sum() // 2."""
    with _Snapshot(x, edges, device_id) as s:
        return s.q.crossings(rows)[0].astype(np.int64)


def edge_crossings(x, edges=None, device_id=None):
    """The exact number of crossing pairs of edges, an int."""
    with _Snapshot(x, edges, device_id) as s:
        return s.q.crossings()[1] // 2


def estimate_edge_crossings(x, edges=None, sample_size=4096, seed=0, device_id=None):
    """(estimate, standard_error) of the crossing number from S = min(sample_size, E) edges drawn without replacement,
    rows = sort(default_rng(seed).choice(E, S, replace=False)): estimate = E / (2 S) * sum(counts), standard error =
    E / 2 * std(counts, ddof=1) / sqrt(S) * sqrt(1 - S / E) (0.0 when S = E or S < 2).  With S = E the estimate is the
    exact total."""
    with _Snapshot(x, edges, device_id) as s:
        return s.estimate(sample_size, seed)


def edge_length_stats(x, edges=None, device_id=None):
    """dict(min, max, mean, std) of the edge lengths over all D coordinates, in float64; std is the population value
    sqrt(sum L^2 / E - mean^2).  Without edges: min = inf, max = -inf, mean = std = nan."""
    with _Snapshot(x, edges, device_id) as s:
        return s.length_stats()


def layout_quality(x, edges=None, exact=None, sample_size=4096, seed=0, device_id=None):
    """dict: n_edges, crossings, crossings_stderr (0.0 when exact), crossings_exact, crossings_per_edge
    (2 * crossings / E), min / max / mean / std of the edge lengths, and L_min when x is an embedder.

    exact=True counts every pair, exact=False estimates from `sample_size` edges (estimate_edge_crossings); exact=None
    counts exactly up to EXACT_MAX_EDGES edges (HOST_EXACT_MAX_EDGES on the host path) and estimates above, which keeps
    the call under about a second."""
    with _Snapshot(x, edges, device_id) as s:
        E = s.q.E
        if exact is None:
            exact = E <= (EXACT_MAX_EDGES if s.q.device_id >= 0 else HOST_EXACT_MAX_EDGES)
        if exact:
            crossings, stderr = s.q.crossings()[1] // 2, 0.0
        else:
            crossings, stderr = s.estimate(sample_size, seed)
            exact = min(int(sample_size), E) == E
        out = {"n_edges": E, "crossings": crossings, "crossings_stderr": stderr, "crossings_exact": bool(exact),
               "crossings_per_edge": 2 * crossings / E if E else 0.0}
        out.update(s.length_stats())
        if s.L_min is not None:
            out["L_min"] = s.L_min
        return out


# ---- embedding quality: neighbour ranks and what is computed from them ----------------------------------------------------
def neighbor_ranks(x, edges=None, rows=None, device_id=None):
    """For the source vertex ids `rows` (any order, repeats allowed; None = all vertices in order), in CSR form: dict of
    sources (int64), indptr (int64, len(sources) + 1), and per slot neighbors (int32, the distinct neighbours of the source
    in the simple graph, ids ascending), dist2 (float32, d2(source, neighbour) under the header's float32 chain), below and
    equal (int64): how many vertices other than the source and that neighbour lie strictly nearer to the source than the
    neighbour, and how many exactly as near.  Neighbours and non-neighbours are counted alike."""
    with _Snapshot(x, edges, device_id) as s:
        return s.ranks(rows)


def _non_neighbor_counts(r):
    """(k per slot, b_bar, q_bar): the counts of a slot among the NON-neighbours only.  The counts among the source's other
    neighbours come from dist2 within the row -- b_N = #{v' in N(u), v' != v: d2(u, v') < d2(u, v)}, q_N likewise for
    equality -- and b_bar = below - b_N, q_bar = equal - q_N."""
    indptr, d2 = r["indptr"], r["dist2"]
    k = np.diff(indptr)
    row = np.repeat(np.arange(len(k), dtype=np.uint64), k)
    if len(d2) == 0:
        return k[:0], r["below"], r["equal"]
    # one sort by (row, distance): a distance is >= +0, +inf or the one NaN 0x7FC00000, and on those the float32 bits order
    # as the values do, NaN last
    order = np.argsort((row << np.uint64(32)) | d2.view(np.uint32), kind="stable")
    sd, srow = d2[order], row[order]
    idx = np.arange(len(sd))
    new_row = np.r_[True, srow[1:] != srow[:-1]]
    new_val = new_row | np.r_[True, sd[1:] != sd[:-1]]   # NaN != NaN: every NaN is a group of its own
    row_start = np.maximum.accumulate(np.where(new_row, idx, 0))
    val_start = np.maximum.accumulate(np.where(new_val, idx, 0))
    group = np.cumsum(new_val) - 1
    b_n, q_n = np.zeros(len(sd), dtype=np.int64), np.zeros(len(sd), dtype=np.int64)
    b_n[order] = np.where(np.isnan(sd), 0, val_start - row_start)   # nothing is below a NaN
    q_n[order] = np.bincount(group)[group] - 1
    return np.repeat(k, k), r["below"] - b_n, r["equal"] - q_n


def _link_auc(counts, n):
    k, b_bar, q_bar = counts
    m = n - 1 - k
    use = m >= 1
    den = 2 * int(np.sum(m[use]))                    # sum over slots of 2 m_u = sum over sources of 2 k_u m_u
    if den == 0:
        return float("nan")
    num = den - 2 * int(np.sum(b_bar[use])) - int(np.sum(q_bar[use]))   # sum of 2 (m - b_bar - q_bar) + q_bar, in Python integers
    return num / den


def _preservation(r):
    k = np.diff(r["indptr"])
    row = np.repeat(np.arange(len(k)), k)
    h = np.bincount(row[r["below"] < k[row]], minlength=len(k)).astype(np.int64)
    has = k >= 1
    if not has.any():
        return {"precision": float("nan"), "jaccard": float("nan")}
    return {"precision": int(h.sum()) / int(k.sum()), "jaccard": float(np.mean(h[has] / (2 * k[has] - h[has])))}


def link_auc(x, edges=None, rows=None, device_id=None):
    """Link-reconstruction AUC: the probability that a neighbour of a source lies nearer to it than a non-neighbour, a tie
    counted one half, pooled over the sources in `rows` (None: all) that have a neighbour and a non-neighbour (k_u >= 1,
    m_u = n - 1 - k_u >= 1): sum over slots of 2 (m_u - b_bar - q_bar) + q_bar, divided by sum over sources of 2 k_u m_u --
    exact integers and one float64 division.  A non-neighbour at a NaN distance counts as farther.  nan when no source
    qualifies."""
    with _Snapshot(x, edges, device_id) as s:
        return _link_auc(_non_neighbor_counts(s.ranks(rows)), s.q.n)


def neighborhood_preservation(x, edges=None, rows=None, device_id=None):
    """dict(precision, jaccard): how much of N(u) is among the k_u vertices nearest to u.  h_u = #{v in N(u): below(u -> v) <
    k_u}: a neighbour is kept when fewer than k_u other vertices are STRICTLY nearer, so ties count in the neighbour's
    favour.  precision = sum h_u / sum k_u (one division of integers); jaccard = the mean over the sources with k_u >= 1 of
    h_u / (2 k_u - h_u).  nan for both when no source has a neighbour."""
    with _Snapshot(x, edges, device_id) as s:
        return _preservation(s.ranks(rows))


def embedding_quality(x, edges=None, exact=None, sample_size=4096, seed=0, device_id=None):
    """dict: n_vertices, sources (how many source vertices were used), sources_exact (every vertex was one), link_auc,
    neighborhood_precision, neighborhood_jaccard (link_auc and neighborhood_preservation over those sources) and mean_rank
    (the mean over slots of b_bar, the number of non-neighbours strictly nearer than the neighbour; nan without slots).

    exact=True takes every vertex as a source; exact=False takes S = min(sample_size, n) of them, rows =
    sort(default_rng(seed).choice(n, S, replace=False)); exact=None takes all up to EXACT_MAX_VERTICES vertices
    (HOST_EXACT_MAX_VERTICES on the host path) and samples above."""
    with _Snapshot(x, edges, device_id) as s:
        n = s.q.n
        rows = s.sample(exact, sample_size, seed)
        r = s.ranks(rows)
        counts = _non_neighbor_counts(r)
        b_bar = counts[1]
        pres = _preservation(r)
        return {"n_vertices": n, "sources": len(r["sources"]), "sources_exact": rows is None,
                "link_auc": _link_auc(counts, n), "neighborhood_precision": pres["precision"],
                "neighborhood_jaccard": pres["jaccard"],
                "mean_rank": int(b_bar.sum()) / len(b_bar) if len(b_bar) else float("nan")}


# ---- distance preservation: the hop profile and what is computed from it ---------------------------------------------------
def hop_profile(x, edges=None, sources=None, device_id=None):
    """The sums of include/graphem_hip.h "distance preservation" over the source vertex ids `sources` (any order, repeats
    allowed; None = all vertices in order) on the SIMPLE graph of the edge list: dict of sources (int64), hops =
    arange(1, H + 1), and per hop pairs (int64: the (source, vertex) pairs at that hop), sum_d and sum_d2 (float64: the sums
    of the embedding distance and of its square over them), min_d2 and max_d2 (float32, exact), mean_d = sum_d / pairs (the
    Shepard curve); per source reach (int64: the vertices it reaches, itself not counted), eccentricity (int32),
    sum_d_over_h and sum_d2_over_h2 (float64: the sums over the vertices it reaches of d / hop and d^2 / hop^2); and
    n_unreachable = S (n - 1) - sum(reach)."""
    with _Snapshot(x, edges, device_id) as s:
        return s.hops(sources)


def _stress(p, scale=None):
    """layout_stress's dict from a hop profile: stress(s) = (s^2 B - 2 s A + N) / N."""
    a, b, c = p["sum_d_over_h"], p["sum_d2_over_h2"], p["reach"]
    A, B, N = math.fsum(a), math.fsum(b), int(c.sum())
    if scale is None:
        scale = A / B if B > 0 else 1.0
    s = float(scale)
    t = s * s * b - 2 * s * a + c
    with np.errstate(invalid="ignore", divide="ignore"):
        vertex = np.where(c > 0, t / c, np.nan)
    return {"stress": (s * s * B - 2 * s * A + N) / N if N else float("nan"), "scale": s, "pairs": N,
            "n_unreachable": p["n_unreachable"], "sources": p["sources"], "vertex_stress": vertex}, t


def layout_stress(x, edges=None, sources=None, scale=None, device_id=None):
    """Kamada-Kawai stress of the layout against hop distance with the weights 1 / hop^2, over the pairs P of hop_profile:
    stress(s) = sum over P of (s d - hop)^2 / hop^2, divided by |P| = (s^2 B - 2 s A + N) / N with A = sum of sum_d_over_h,
    B = sum of sum_d2_over_h2, N = sum of reach.  scale=None takes the minimiser s* = A / B (1.0 when B = 0).  dict: stress
    (nan when N = 0), scale, pairs = N, n_unreachable, sources, and vertex_stress, the same quotient over one source's pairs
    (nan for a source that reaches nothing): which vertices are badly placed."""
    with _Snapshot(x, edges, device_id) as s:
        return _stress(s.hops(sources), scale)[0]


def _hop_correlation(p):
    h = p["hops"].astype(np.float64)
    n = int(p["pairs"].sum())
    if n == 0:
        return float("nan")
    sh, shh = math.fsum(h * p["pairs"]), math.fsum(h * h * p["pairs"])
    shd, sd, sdd = math.fsum(h * p["sum_d"]), math.fsum(p["sum_d"]), math.fsum(p["sum_d2"])
    var_h, var_d = n * shh - sh * sh, n * sdd - sd * sd
    if not (var_h > 0 and var_d > 0):
        return float("nan")
    return (n * shd - sh * sd) / math.sqrt(var_h * var_d)


def hop_distance_correlation(x, edges=None, sources=None, device_id=None):
    """Pearson's r between hop distance and embedding distance over the pairs P of hop_profile, from the per-hop table:
    sum h = sum h pairs[h], sum h^2 = sum h^2 pairs[h], sum h d = sum h sum_d[h], sum d = sum sum_d[h], sum d^2 = sum sum_d2[h].
    nan when either variance is 0 (no pairs, one hop only, all distances equal)."""
    with _Snapshot(x, edges, device_id) as s:
        return _hop_correlation(s.hops(sources))


def distance_quality(x, edges=None, exact=None, sample_size=1024, seed=0, device_id=None):
    """dict: n_sources, exact (every vertex was a source), pairs, n_unreachable, stress and scale (layout_stress at its
    minimiser), stress_stderr, correlation (hop_distance_correlation), hops, mean_d (the Shepard curve) and max_hop.

    exact=True takes every vertex as a source; exact=False takes S = min(sample_size, n) of them, sources =
    sort(default_rng(seed).choice(n, S, replace=False)); exact=None takes all up to EXACT_MAX_DISTANCE_VERTICES vertices
    (HOST_EXACT_MAX_DISTANCE_VERTICES on the host path) and samples above.  stress_stderr is 0.0 when exact or S < 2, else
    the ratio estimator's error: with t_j = s^2 b_j - 2 s a_j + c_j and c_j = reach[j],
    sqrt(S / (S - 1) * sum_j (t_j - stress c_j)^2) / sum_j c_j * sqrt(1 - S / n)."""
    with _Snapshot(x, edges, device_id) as s:
        n = s.q.n
        sources = s.distance_sample(exact, sample_size, seed)
        p = s.hops(sources)
        st, t = _stress(p)
        S = len(p["sources"])
        stderr = 0.0
        if sources is not None and S >= 2 and st["pairs"] > 0:
            resid = t - st["stress"] * p["reach"]
            stderr = math.sqrt(S / (S - 1) * math.fsum(resid * resid)) / st["pairs"] * math.sqrt(1 - S / n)
        return {"n_sources": S, "exact": sources is None, "pairs": st["pairs"], "n_unreachable": p["n_unreachable"],
                "stress": st["stress"], "scale": st["scale"], "stress_stderr": stderr, "correlation": _hop_correlation(p),
                "hops": p["hops"], "mean_d": p["mean_d"], "max_hop": len(p["hops"])}
