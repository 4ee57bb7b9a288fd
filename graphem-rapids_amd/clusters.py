"""Clusters of an embedding on the GPU: exact k-means, the silhouette, and how well the clusters recover given labels.

The package embeds a graph, finds communities on the graph itself (communities.py) and plants them (generate_sbm(labels=True),
the caveman families, planted_partition_edges).  This module asks the question those lead to: do the clusters of the
embedding equal the communities of the graph?  It is also the second half of spectral clustering: k-means on Laplacian
eigenvectors.

The rule is include/graphem_hip.h "embedding clusters".  The distance is the float32 chain of the embedding-quality measures
over all D coordinates; a vertex takes the least centre id among the nearest; and a centre is the quotient of an INTEGER sum
of quantised coordinates by the member count, so labels, distances, counts and the centres' bits are a pure function of
(positions, start centres, max_iter): they do not depend on launch geometry, on the order of atomic adds, on vertex order, or
on whether the kernels (csrc/clusters.hip) or the library's host path (device_id < 0) ran.  It is a float32 rule: a float64
embedder's positions are rounded to float32 first.

Every function takes either a GraphEmbedderHIP, whose device positions are used in place (no download), or an (n, D) array
or tensor.  The silhouette is that of scikit-learn (Euclidean), from per-cluster distance sums computed on the device.
"""
import math

import numpy as np

from . import _native
from .communities import adjusted_rand_index, normalized_mutual_info
from .quality import _default_device

MAX_CLUSTERS = 4096   # the library's bound on k
# silhouette_score(exact=None) takes every vertex as a row up to this many vertices and samples rows above it.  Measured on
# one MI355X (2026-10-19, tools/cluster_quality.py --blocks 16 --n-per-block 6250 --iters 20 --time --host --all and
# --n-per-block 15625 --iters 20 --time --all --no-louvain --repeats 2; an SBM of 16 blocks, D = 3, the layout after 20
# iterations, k = 16): the distance sums over all rows take 0.0239 s at 100 K vertices and 0.161 s at
# 250 K, 4.2e11 and 3.9e11 (row, column) pairs per second, and the time grows with the square of n: 2.58e-12 n^2 is a second
# at 620 000 vertices (no all-rows run above 250 K stands behind that).  4096 sampled rows take 1.5 ms at 100 K and 12.6 ms at
# a million.
EXACT_MAX_SILHOUETTE_VERTICES = 600_000
# The same for the library's host path (no device): 256 rows take 3.3 ms at 100 K and 29.5 ms at a million on 16 threads of
# the same machine's host, 7.8e9 and 8.7e9 pairs per second; all rows were not run there, and at the 100 K rate they take a
# second at 88 000 vertices.
HOST_EXACT_MAX_SILHOUETTE_VERTICES = 80_000


class _Points:
    """A LayoutQuality handle without edges holding the positions of `x`: with-statement owner of the native handle."""

    def __init__(self, x, device_id=None):
        no_edges = np.zeros((0, 2), dtype=np.int32)
        engine = getattr(x, "_engine", None)
        if engine is not None:
            on_device = device_id is None or device_id >= 0
            self.q = _native.LayoutQuality(no_edges, x.n, x.device.index if on_device else device_id)
            try:
                if engine.f64 or not on_device:
                    self.q.set_positions(engine.get_positions().astype(np.float32))   # the rule is a float32 rule
                else:
                    self.q.set_positions_device(engine.positions_unpadded_device_ptr(), engine.D)
            except Exception:
                self.q.close()
                raise
            return
        pos = np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x)
        if pos.ndim != 2:
            raise ValueError(f"positions must be (n, D), got shape {pos.shape}")
        self.q = _native.LayoutQuality(no_edges, pos.shape[0], _default_device() if device_id is None else device_id)
        try:
            self.q.set_positions(pos.astype(np.float32))
        except Exception:
            self.q.close()
            raise

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.q.close()

    def check_k(self, k):
        top = min(self.q.n, MAX_CLUSTERS)
        if not isinstance(k, (int, np.integer)) or k < 1 or k > top:
            raise ValueError(f"k must be in [1, min(n, {MAX_CLUSTERS})] = [1, {top}], got {k}")
        return int(k)

    def plusplus(self, k, seed):
        """kmeans_plusplus' ids."""
        n = self.q.n
        rng = np.random.default_rng(seed)
        ids = [int(rng.integers(n))]
        chosen = np.zeros(n, dtype=bool)
        chosen[ids[0]] = True
        while len(ids) < k:
            min_d2 = self.q.kmeans_seed_step(ids[-1], len(ids) == 1)
            cs = np.cumsum(min_d2.astype(np.float64))
            if cs[-1] > 0:
                i = int(np.searchsorted(cs, rng.random() * cs[-1], side="right"))
                if i >= n:
                    i = int(np.flatnonzero(min_d2 > 0)[-1])
            else:
                i = int(np.flatnonzero(~chosen)[0])
            ids.append(i)
            chosen[i] = True
        return np.array(ids, dtype=np.int64)

    def start(self, k, init, seed):
        """The (k, D) float32 start centres of one run."""
        if isinstance(init, str):
            if init == "k-means++":
                ids = self.plusplus(k, seed)
            elif init == "random":
                ids = np.sort(np.random.default_rng(seed).choice(self.q.n, k, replace=False))
            else:
                raise ValueError(f"init must be 'k-means++', 'random' or a (k, D) array, got {init!r}")
            return self.q.position_rows(ids)
        centres = np.asarray(init.detach().cpu().numpy() if hasattr(init, "detach") else init, dtype=np.float32)
        if centres.shape != (k, self.q.D):
            raise ValueError(f"init must be ({k}, {self.q.D}), got {centres.shape}")
        return centres

    def kmeans(self, k, init, n_init, max_iter, seed):
        k = self.check_k(k)
        best = None
        for run in range(max(int(n_init), 1) if isinstance(init, str) else 1):
            r = self.q.kmeans(self.start(k, init, seed + run), max_iter)
            r["inertia"] = math.fsum(r["d2"].tolist())
            if best is None or r["inertia"] < best["inertia"]:
                best = r
        return {key: best[key] for key in ("labels", "centers", "d2", "counts", "inertia", "n_iter", "converged")}

    def silhouette(self, labels, rows=None):
        """silhouette_samples' values for the vertex ids `rows` (None: all)."""
        n = self.q.n
        labels = np.asarray(labels).ravel()
        if len(labels) != n:
            raise ValueError(f"{len(labels)} labels for {n} vertices")
        inv = np.unique(labels, return_inverse=True)[1].reshape(n)
        k = int(inv.max()) + 1 if n else 0
        if not 2 <= k <= n - 1:
            raise ValueError(f"Number of labels is {k}. Valid values are 2 to n_samples - 1 (inclusive)")
        sums = self.q.cluster_distance_sums(inv, k, rows)
        ids = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64).ravel()
        counts = np.bincount(inv, minlength=k).astype(np.float64)
        own = inv[ids]
        r = np.arange(len(ids))
        with np.errstate(invalid="ignore", divide="ignore"):
            a = sums[r, own] / (counts[own] - 1)
            mean = sums / counts
            mean[r, own] = np.inf
            b = mean.min(axis=1)
            s = (b - a) / np.maximum(a, b)
        s[counts[own] == 1] = 0.0          # a singleton cluster
        return np.where(np.isnan(s), 0.0, s)   # 0 / 0: every point of the vertex's and of the nearest cluster coincides with it

    def sample(self, exact, sample_size, seed):
        """The row ids silhouette_score uses: None (all vertices) or the sorted sample."""
        n = self.q.n
        if exact is None:
            exact = n <= (EXACT_MAX_SILHOUETTE_VERTICES if self.q.device_id >= 0 else HOST_EXACT_MAX_SILHOUETTE_VERTICES)
        S = min(int(sample_size), n)
        if exact or S >= n:
            return None
        return np.sort(np.random.default_rng(seed).choice(n, S, replace=False))


def kmeans_plusplus(x, k, seed=0, device_id=None):
    """int64 (k,): the vertex ids of k-means++ start centres.  rng = default_rng(seed); the first id is
    int(rng.integers(n)); each later one is drawn with probability proportional to min_d2, the float32 squared distance to
    the nearest id chosen so far, kept on the device: cs = cumsum(min_d2 as float64) in vertex order and, while cs[-1] > 0,
    i = searchsorted(cs, rng.random() * cs[-1], side='right') (the last vertex with min_d2 > 0 should the search run off the
    end); when every vertex coincides with a chosen one, the least id not yet chosen.  A chosen vertex is never drawn again.
    The device and the host path give the same min_d2 bits, hence the same ids."""
    with _Points(x, device_id) as p:
        return p.plusplus(p.check_k(k), seed)


def kmeans(x, k, init="k-means++", n_init=1, max_iter=300, seed=0, device_id=None):
    """Lloyd's k-means with exact centre updates.  dict: labels (int32 (n,)), centers (float32 (k, D)), d2 (float32 (n,): the
    squared distance to the vertex's centre), counts (int64 (k,)), inertia = math.fsum(d2), n_iter (the number of centre
    updates) and converged (the labels repeated; False when max_iter updates did not get there).  The labels and d2 always
    belong to the returned centres; a cluster that loses every member keeps its centre.

    init: 'k-means++' (kmeans_plusplus), 'random' (the rows sort(default_rng(seed).choice(n, k, replace=False))) or a (k, D)
    array of start centres.  n_init > 1 runs the seeds seed, seed + 1, ... and keeps the least inertia, the earliest on a tie.
    max_iter = 0 assigns to the start centres.  1 <= k <= min(n, 4096); a NaN or an infinity in a position or a centre
    raises ValueError."""
    with _Points(x, device_id) as p:
        return p.kmeans(k, init, n_init, max_iter, seed)


def nearest_center(x, centers, device_id=None):
    """(labels int32, d2 float32): for every vertex the least id among its nearest rows of `centers` (k, D) and the float32
    squared distance to it."""
    with _Points(x, device_id) as p:
        return p.q.kmeans_assign(centers)


def silhouette_samples(x, labels, rows=None, device_id=None):
    """float64: the silhouette of the vertex ids `rows` (any order, repeats allowed; None = all vertices in order) under the
    Euclidean distance, every one compared against all n vertices: with sums[c] = the sum of the distances to the members of
    cluster c other than the vertex itself, a = sums[own] / (|own| - 1), b = the least sums[c] / |c| over the other clusters,
    s = (b - a) / max(a, b); 0.0 for a vertex alone in its cluster and for 0 / 0.  labels: any integers, n of them.  ValueError
    unless 2 <= number of distinct labels <= n - 1, as in scikit-learn."""
    with _Points(x, device_id) as p:
        return p.silhouette(labels, rows)


def silhouette_score(x, labels, exact=None, sample_size=4096, seed=0, device_id=None):
    """The mean silhouette, a float.  exact=True takes every vertex; exact=False takes S = min(sample_size, n) of them, rows =
    sort(default_rng(seed).choice(n, S, replace=False)), each still compared against all n vertices; exact=None takes all up to
    EXACT_MAX_SILHOUETTE_VERTICES vertices (HOST_EXACT_MAX_SILHOUETTE_VERTICES on the host path) and samples above."""
    with _Points(x, device_id) as p:
        s = p.silhouette(labels, p.sample(exact, sample_size, seed))
        return math.fsum(s.tolist()) / len(s)


def cluster_recovery(x, truth, k=None, n_init=4, max_iter=300, seed=0, init="k-means++", exact=None, sample_size=4096,
                     device_id=None):
    """Do the clusters of the embedding equal the labelling `truth`?  k-means with k clusters (default: the number of distinct
    truth labels) and n_init starts, then dict: k, ari (adjusted_rand_index) and nmi (normalized_mutual_info) of the k-means
    labels against truth, inertia, silhouette of the k-means labels (silhouette_score with exact, sample_size and seed; nan
    when they name fewer than 2 or more than n - 1 clusters), silhouette_exact (every vertex was a row), n_iter, converged
    and labels.  truth: n labels, such as generate_sbm(labels=True)'s or community_labels(G)."""
    truth = np.asarray(truth).ravel()
    with _Points(x, device_id) as p:
        if len(truth) != p.q.n:
            raise ValueError(f"{len(truth)} truth labels for {p.q.n} vertices")
        if k is None:
            k = len(np.unique(truth))
        r = p.kmeans(k, init, n_init, max_iter, seed)
        labels = r["labels"]
        rows = p.sample(exact, sample_size, seed)
        sil = float("nan")
        if 2 <= len(np.unique(labels)) <= p.q.n - 1:
            s = p.silhouette(labels, rows)
            sil = math.fsum(s.tolist()) / len(s)
        return {"k": int(k), "ari": adjusted_rand_index(truth, labels), "nmi": normalized_mutual_info(truth, labels),
                "inertia": r["inertia"], "silhouette": sil, "silhouette_exact": rows is None, "n_iter": r["n_iter"],
                "converged": r["converged"], "labels": labels}
