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
"""
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
