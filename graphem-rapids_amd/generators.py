"""Scale-capable synthetic graphs.

The reference builds its inputs with NetworkX (graphem_rapids/generators.py:32-49,
235-252), which is O(n^2) for G(n, p) and ~8 s per 100 K vertices for random-regular
graphs.  These generators are O(E), vectorised numpy, and return the same thing the
reference's do: a symmetric scipy CSR adjacency matrix with integer ones.

The reference's other eleven families follow below, none through NetworkX.  Block model (generate_sbm,
generate_bipartite_graph), random geometric graph and preferential attachment are counter-based rules
(include/graphem_hip.h "graph generators") run by HIP kernels when a device is present and the input is past the
crossover size, else by the library's host path: the same edges bit for bit either way, so the choice is invisible.
Caveman, grid and balanced tree are closed forms equal to networkx's edge for edge; Watts-Strogatz, Holme-Kim,
the directed scale-free process and the relaxed caveman graph mirror networkx's processes step by step in O(E)
host code on numpy.random.default_rng(seed) -- the same distributions, not networkx's streams.
"""
import numpy as np
import scipy.sparse as sp


def edges_to_adjacency(n, edges):
    """(E, 2) undirected edge list -> symmetric CSR of ones (what _nx_to_sparse_adjacency returns)."""
    edges = np.asarray(edges).reshape(-1, 2)
    if len(edges) == 0:
        return sp.csr_matrix((n, n), dtype=np.int64)
    rows = np.concatenate([edges[:, 0], edges[:, 1]])
    cols = np.concatenate([edges[:, 1], edges[:, 0]])
    adj = sp.csr_matrix((np.ones(len(rows), dtype=np.int64), (rows, cols)), shape=(n, n))
    adj.sum_duplicates()
    adj.data[:] = 1
    return adj


def erdos_renyi_edges(n, p, seed=0):
    """G(n, p) by geometric skipping over the n(n-1)/2 vertex pairs: O(E) work.
    Returns (E, 2) int64 with u < v, sorted by (u, v)."""
    rng = np.random.default_rng(seed)
    total = n * (n - 1) // 2
    if p <= 0 or total == 0:
        return np.zeros((0, 2), dtype=np.int64)
    if p >= 1:
        iu = np.triu_indices(n, 1)
        return np.column_stack(iu).astype(np.int64)
    expected = total * p
    chunks, pos = [], -1
    while True:
        m = int(expected * 1.1 + 1000)
        gaps = rng.geometric(p, size=m).astype(np.int64)
        idx = pos + np.cumsum(gaps)
        over = np.searchsorted(idx, total)
        chunks.append(idx[:over])
        if over < m:
            break
        pos = int(idx[-1])
        expected = (total - pos) * p
    lin = np.concatenate(chunks)
    # linear index -> (u, v) in the strictly upper triangle, row-major
    nn = float(n)
    u = np.floor(((2 * nn - 1) - np.sqrt((2 * nn - 1) ** 2 - 8.0 * lin)) / 2).astype(np.int64)
    start = u * (2 * n - u - 1) // 2
    bad = start > lin          # fix the rare off-by-one of the float sqrt
    u[bad] -= 1
    start = u * (2 * n - u - 1) // 2
    nxt = (u + 1) * (2 * n - u - 2) // 2
    bad = lin >= nxt
    u[bad] += 1
    start = u * (2 * n - u - 1) // 2
    v = lin - start + u + 1
    return np.column_stack([u, v])


def erdos_renyi_graph(n, p, seed=0):
    """Same signature as the reference's erdos_renyi_graph (generators.py:32-49); a different
    random stream (numpy instead of NetworkX), the same distribution."""
    return edges_to_adjacency(n, erdos_renyi_edges(n, p, seed))


def random_regular_edges(n, d, seed=0, max_rounds=200):
    """d-regular simple graph by the pairing model with local repair: stubs are paired at
    random; pairs that are loops or repeats are dissolved together with an equal number of
    random good pairs and re-paired.  O(n d) per round, a handful of rounds in practice."""
    if (n * d) % 2 != 0:
        raise ValueError("n * d must be even")
    if d >= n:
        raise ValueError("d must be smaller than n")
    rng = np.random.default_rng(seed)
    good = np.zeros((0, 2), dtype=np.int64)
    stubs = np.repeat(np.arange(n, dtype=np.int64), d)
    for _ in range(max_rounds):
        stubs = rng.permutation(stubs)
        u, v = stubs[0::2], stubs[1::2]
        lo, hi = np.minimum(u, v), np.maximum(u, v)
        cand = np.column_stack([lo, hi])
        allp = np.vstack([good, cand])
        key = allp[:, 0] * n + allp[:, 1]
        order = np.argsort(key, kind="stable")
        sk = key[order]
        dup_sorted = np.zeros(len(sk), dtype=bool)
        dup_sorted[1:] = sk[1:] == sk[:-1]      # later copies of a repeated pair
        dup = np.zeros(len(sk), dtype=bool)
        dup[order] = dup_sorted
        bad = dup | (allp[:, 0] == allp[:, 1])
        bad[:len(good)] = False                  # established pairs stay
        good = allp[~bad]
        rest = allp[bad]
        if len(rest) == 0:
            order = np.lexsort((good[:, 1], good[:, 0]))
            return good[order]
        # dissolve as many random good pairs as there are bad ones so repair can succeed
        take = min(len(good), max(len(rest), 8))
        pick = rng.choice(len(good), size=take, replace=False)
        mask = np.ones(len(good), dtype=bool)
        mask[pick] = False
        stubs = np.concatenate([rest.ravel(), good[pick].ravel()])
        good = good[mask]
    raise RuntimeError("random_regular_edges did not converge")


def planted_partition_edges(n, communities, deg_in, deg_out, seed=0, shuffle=True):
    """A graph WITH structure for locality experiments (SNAP-like: dense communities, sparse links between them):
    `communities` equal blocks; about n * deg_in / 2 random pairs inside blocks and n * deg_out / 2 random pairs anywhere;
    loops and repeats dropped.  shuffle: vertex numbers permuted at random, so that the numbering says nothing about
    the blocks (an engine has to find the locality itself).  Returns (E, 2) int64 with u < v, sorted by (u, v)."""
    rng = np.random.default_rng(seed)
    size = n // communities
    m_in, m_out = int(n * deg_in / 2), int(n * deg_out / 2)
    u = rng.integers(0, size * communities, size=m_in)
    v = (u // size) * size + rng.integers(0, size, size=m_in)
    a = np.concatenate([u, rng.integers(0, n, size=m_out)])
    b = np.concatenate([v, rng.integers(0, n, size=m_out)])
    if shuffle:
        perm = rng.permutation(n)
        a, b = perm[a], perm[b]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    keep = lo != hi
    key = np.unique(lo[keep] * n + hi[keep])
    return np.column_stack([key // n, key % n])


def generate_random_regular(n=100, d=3, seed=0):
    """Same signature as the reference's generate_random_regular (generators.py:235-252)."""
    return edges_to_adjacency(n, random_regular_edges(n, d, seed))


def load_snap_edge_list(path, directed=False, relabel=True):
    """SNAP text edge list -> (vertices, edges), the format and the rules of the reference's
    SNAPDataset.load() (datasets.py:306-357): lines starting with '#' are comments, a row is
    'src<ws>dst' (further columns ignored, rows with fewer than two fields skipped); an undirected
    dataset (directed=False) becomes the sorted unique pairs with u < v (self-loops and repeats in
    either direction drop out), a directed one keeps its rows as they come; vertices = the sorted
    labels that occur in the edges.

    relabel=False returns exactly what the reference's loader returns (original labels).
    relabel=True (default) compacts the labels to 0..n-1 in sorted-label order -- what the
    reference's load_dataset_as_networkx does next with convert_node_labels_to_integers
    (datasets.py:761-782) -- so that `edges` indexes an n x n adjacency directly; `vertices` is then
    arange(n).  No download, no NetworkX, no Python-level pair handling (vectorised numpy)."""
    src, dst = [], []
    with open(path, "r", encoding="utf-8") as fh:
        for line in fh:
            if line.startswith("#"):
                continue
            parts = line.strip().split()
            if len(parts) >= 2:
                src.append(int(parts[0]))
                dst.append(int(parts[1]))
    edges = np.column_stack([np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)]).reshape(-1, 2)
    if not directed and len(edges):
        lo, hi = np.minimum(edges[:, 0], edges[:, 1]), np.maximum(edges[:, 0], edges[:, 1])
        keep = lo != hi
        edges = np.unique(np.column_stack([lo[keep], hi[keep]]), axis=0)
    vertices = np.unique(edges.ravel())
    if relabel:
        edges = np.searchsorted(vertices, edges)
        vertices = np.arange(len(vertices), dtype=np.int64)
    return vertices, edges


# ---- counter-based families: HIP kernels or the library's host path (same bits) --------------------------------------
# Below these sizes the host path is taken even with a device present: a device call costs a stream, a dozen
# allocations and several launches before the first edge, more than a small graph takes on the host.
DEVICE_MIN_VERTICES = 20000
_MASK64 = 0xFFFFFFFFFFFFFFFF
_device_count = None


def _generator(size):
    """A _native.Generator on device 0 when one is present and `size` is past the crossover, else on the host path."""
    global _device_count
    from . import _native
    if _device_count is None:
        _device_count = int(_native.load().gh_device_count())
    return _native.Generator(0 if _device_count > 0 and size >= DEVICE_MIN_VERTICES else -1)


def sbm_edges(sizes, p_matrix, seed=0):
    """Stochastic block model: blocks of sizes[a] consecutive vertices, the pair (u, v) of blocks (a, b) an edge
    independently with probability p_matrix[a][b] (symmetric).  O(E + pairs / 16384) by geometric skipping
    (include/graphem_hip.h).  Returns (E, 2) int64 with u < v, sorted by (u, v)."""
    sizes = np.asarray(sizes, dtype=np.int64).ravel()
    P = np.asarray(p_matrix, dtype=np.float64)
    if P.shape != (len(sizes), len(sizes)) and (len(sizes) or P.size):
        raise ValueError("p_matrix must be (blocks, blocks)")
    if (sizes < 0).any():
        raise ValueError("block sizes must be >= 0")
    if not ((P >= 0) & (P <= 1)).all():
        raise ValueError("probabilities must be in [0, 1]")
    if not np.array_equal(P, P.T):
        raise ValueError("p_matrix must be symmetric")
    g = _generator(int(sizes.sum()))
    try:
        return g.sbm(sizes, P, int(seed) & _MASK64).astype(np.int64)
    finally:
        g.close()


def geometric_edges(n, radius, dim=2, seed=0, return_positions=False):
    """Random geometric graph on n uniform points of the unit cube (coordinates k / 2^24): (u, v) is an edge iff their
    distance is <= radius, decided on the integer coordinates (include/graphem_hip.h).  1 <= dim <= 8.  Returns (E, 2)
    int64 with u < v, sorted by (u, v); with return_positions also the (n, dim) float32 positions."""
    if n < 0:
        raise ValueError("n must be >= 0")
    if not 1 <= dim <= 8:
        raise ValueError("dim must be in [1, 8]")
    if not radius >= 0:
        raise ValueError("radius must be >= 0")
    g = _generator(int(n))
    try:
        edges, pos = g.geometric(n, radius, dim, int(seed) & _MASK64)
    finally:
        g.close()
    edges = edges.astype(np.int64)
    return (edges, pos) if return_positions else edges


def barabasi_albert_edges(n, m, seed=0, return_rounds=False):
    """Preferential attachment as networkx 3.x runs it: the star on 0 .. m, then every vertex draws from the endpoint
    list of all earlier edges until it holds m distinct targets (include/graphem_hip.h).  E = m (n - m).  Returns
    (E, 2) int64 with u < v, sorted by (u, v); with return_rounds also the number of dependency rounds the device took
    (0 on the host path)."""
    if m < 1 or m >= n:
        raise ValueError(f"Barabasi-Albert network must have m >= 1 and m < n, m = {m}, n = {n}")
    g = _generator(int(n))
    try:
        edges = g.ba(n, m, int(seed) & _MASK64).astype(np.int64)
        rounds = g.rounds
    finally:
        g.close()
    return (edges, rounds) if return_rounds else edges


def generate_sbm(n_per_block=75, num_blocks=4, p_in=0.15, p_out=0.01, labels=False, seed=0):
    """Same signature as the reference's generate_sbm (generators.py:67-109): num_blocks blocks of n_per_block vertices,
    p_in inside a block and p_out between blocks; with labels=True also the block id of every vertex."""
    P = np.full((num_blocks, num_blocks), float(p_out))
    np.fill_diagonal(P, float(p_in))
    adjacency = edges_to_adjacency(n_per_block * num_blocks, sbm_edges([n_per_block] * num_blocks, P, seed))
    if labels:
        return adjacency, np.repeat(np.arange(num_blocks), n_per_block)
    return adjacency


def bipartite_edges(n_top, n_bottom, p=0.1, seed=0):
    """Random bipartite graph: top vertices 0 .. n_top-1, bottom ones after them, every top-bottom pair an edge with
    probability p -- the block model of two blocks with an empty diagonal."""
    return sbm_edges([n_top, n_bottom], [[0.0, p], [p, 0.0]], seed)


def generate_bipartite_graph(n_top=50, n_bottom=100, *, seed=None):
    """Same positional signature as the reference's generate_bipartite_graph (generators.py:199-214; p = 0.1).  The
    reference is unseeded; seed=None draws a fresh seed, an int makes the graph reproducible."""
    if seed is None:
        seed = int(np.random.SeedSequence().entropy) & _MASK64
    return edges_to_adjacency(n_top + n_bottom, bipartite_edges(n_top, n_bottom, 0.1, seed))


def generate_geometric(n=100, radius=0.2, dim=2, seed=0):
    """Same signature as the reference's generate_geometric (generators.py:280-299)."""
    return edges_to_adjacency(n, geometric_edges(n, radius, dim, seed))


def generate_ba(n=300, m=3, seed=0):
    """Same signature as the reference's generate_ba (generators.py:112-129)."""
    return edges_to_adjacency(n, barabasi_albert_edges(n, m, seed))


# ---- closed forms: networkx's graphs edge for edge, vertex numbering included ------------------------------------------
def _canonical(n, u, v):
    """Pairs -> (E, 2) int64 with u < v, loops and repeats dropped, sorted by (u, v)."""
    u, v = np.asarray(u, dtype=np.int64).ravel(), np.asarray(v, dtype=np.int64).ravel()
    lo, hi = np.minimum(u, v), np.maximum(u, v)
    key = np.unique(lo[lo != hi] * max(int(n), 1) + hi[lo != hi])
    return np.column_stack([key // max(int(n), 1), key % max(int(n), 1)])


def caveman_edges(l, k):
    """networkx.caveman_graph(l, k): l cliques, clique c on the vertices c k .. c k + k - 1."""
    iu, iv = np.triu_indices(k, 1)
    base = (np.arange(l, dtype=np.int64) * k)[:, None]
    return _canonical(l * k, base + iu[None, :], base + iv[None, :])


def generate_caveman(l=10, k=10):
    """Same signature as the reference's generate_caveman (generators.py:302-317)."""
    return edges_to_adjacency(l * k, caveman_edges(l, k))


def road_network_edges(width, height):
    """networkx.grid_2d_graph(width, height) relabelled in node order as the reference does: (i, j) -> i height + j."""
    ids = np.arange(width * height, dtype=np.int64).reshape(width, height)
    u = np.concatenate([ids[:-1, :].ravel(), ids[:, :-1].ravel()])
    v = np.concatenate([ids[1:, :].ravel(), ids[:, 1:].ravel()])
    return _canonical(width * height, u, v)


def generate_road_network(width=30, height=30):
    """Same signature as the reference's generate_road_network (generators.py:176-196)."""
    return edges_to_adjacency(width * height, road_network_edges(width, height))


def balanced_tree_vertices(r, h):
    """Vertices of networkx.balanced_tree(r, h): (r^(h+1) - 1) / (r - 1), h + 1 for r = 1."""
    return h + 1 if r == 1 else (r ** (h + 1) - 1) // (r - 1)


def balanced_tree_edges(r, h):
    """networkx.balanced_tree(r, h): the children of v are r v + 1 .. r v + r."""
    if r < 1 or h < 0:
        raise ValueError("r must be >= 1 and h >= 0")
    n = balanced_tree_vertices(r, h)
    child = np.arange(1, n, dtype=np.int64)
    return _canonical(n, (child - 1) // r, child)


def generate_balanced_tree(r=2, h=10):
    """Same signature as the reference's generate_balanced_tree (generators.py:217-232)."""
    return edges_to_adjacency(balanced_tree_vertices(r, h), balanced_tree_edges(r, h))


# ---- sequential processes: networkx's steps on numpy.random.default_rng(seed) -------------------------------------------
class _Draws:
    """Uniform draws from a numpy Generator, taken in blocks (a call into numpy per draw would dominate these loops)."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.buf, self.i = [], 0

    def random(self):
        if self.i == len(self.buf):
            self.buf, self.i = self.rng.random(4096).tolist(), 0
        self.i += 1
        return self.buf[self.i - 1]

    def below(self, n):
        """Uniform integer in [0, n)."""
        return min(int(self.random() * n), n - 1)

    def choice(self, seq):
        return seq[self.below(len(seq))]


def _check_probability(p, name="p"):
    if not 0 <= p <= 1:
        raise ValueError(f"{name} must be in [0, 1], {name} = {p}")


def watts_strogatz_edges(n, k, p, seed=0):
    """networkx.watts_strogatz_graph as a process: the ring lattice of k // 2 neighbours on each side; then, for every
    distance j and every vertex u in order, the edge (u, u + j) is rewired with probability p to (u, w), w uniform and
    redrawn while it is u or already a neighbour of u (no rewiring when u is joined to everyone).  k == n: the complete
    graph."""
    if k > n:
        raise ValueError("k > n, choose smaller k or larger n")
    _check_probability(p)
    if k == n:
        iu = np.triu_indices(n, 1)
        return np.column_stack(iu).astype(np.int64)
    adj = [set() for _ in range(n)]
    for j in range(1, k // 2 + 1):
        for u in range(n):
            adj[u].add((u + j) % n)
            adj[(u + j) % n].add(u)
    draws = _Draws(seed)
    for j in range(1, k // 2 + 1):
        for u in range(n):
            v = (u + j) % n
            if draws.random() < p:
                w = draws.below(n)
                skip = False
                while w == u or w in adj[u]:
                    w = draws.below(n)
                    if len(adj[u]) >= n - 1:
                        skip = True
                        break
                if not skip and v in adj[u]:
                    adj[u].discard(v)
                    adj[v].discard(u)
                    adj[u].add(w)
                    adj[w].add(u)
    us = [u for u in range(n) for _ in adj[u]]
    vs = [v for u in range(n) for v in adj[u]]
    return _canonical(n, us, vs)


def generate_ws(n=1000, k=6, p=0.3, seed=0):
    """Same signature as the reference's generate_ws (generators.py:132-151)."""
    return edges_to_adjacency(n, watts_strogatz_edges(n, k, p, seed))


def _distinct_draws(seq, m, draws):
    """networkx _random_subset: uniform draws from seq until m distinct values are held (in the order first drawn)."""
    held = []
    while len(held) < m:
        x = draws.choice(seq)
        if x not in held:
            held.append(x)
    return held


def powerlaw_cluster_edges(n, m, p, seed=0):
    """Holme-Kim as networkx.powerlaw_cluster_graph runs it: m isolated start vertices; every new vertex draws m
    distinct preferential targets, links the first, and for each of its other m - 1 links either (with probability p,
    when the last preferential target has a neighbour it is not joined to yet) closes a triangle with such a neighbour
    or links the next preferential target."""
    if m < 1 or n < m:
        raise ValueError(f"must have m >= 1 and m <= n, m = {m}, n = {n}")
    _check_probability(p)
    draws = _Draws(seed)
    nbrs = [[] for _ in range(n)]          # in the order the links were made
    linked = [set() for _ in range(n)]

    def link(a, b):
        if b not in linked[a]:
            nbrs[a].append(b)
            nbrs[b].append(a)
            linked[a].add(b)
            linked[b].add(a)

    repeated = list(range(m))
    for source in range(m, n):
        possible = _distinct_draws(repeated, m, draws)
        target = possible.pop()
        link(source, target)
        repeated.append(target)
        count = 1
        while count < m:
            if draws.random() < p:
                hood = [x for x in nbrs[target] if x not in linked[source] and x != source]
                if hood:
                    x = draws.choice(hood)
                    link(source, x)
                    repeated.append(x)
                    count += 1
                    continue
            target = possible.pop()
            link(source, target)
            repeated.append(target)
            count += 1
        repeated.extend([source] * m)
    us = [u for u in range(n) for _ in nbrs[u]]
    vs = [v for u in range(n) for v in nbrs[u]]
    return _canonical(n, us, vs)


def generate_power_cluster(n=1000, m=3, p=0.5, seed=0):
    """Same signature as the reference's generate_power_cluster (generators.py:154-173)."""
    return edges_to_adjacency(n, powerlaw_cluster_edges(n, m, p, seed))


def scale_free_edges(n, alpha=0.41, beta=0.54, gamma=0.05, delta_in=0.2, delta_out=0, seed=0, return_vertices=False):
    """The directed process of Bollobas et al. as networkx.scale_free_graph runs it -- from the 3-cycle, each step adds
    with probability alpha a new vertex with an arc to an old one chosen by in-degree + delta_in, with probability
    beta an arc between old vertices (by out-degree + delta_out, by in-degree + delta_in), else a new vertex with an
    arc from an old one -- until there are n vertices; then undirected with self-loops removed, as the reference does.
    Parallel arcs collapse into one edge.  The graph has max(n, 3) vertices."""
    if alpha <= 0 or beta <= 0 or gamma <= 0:
        raise ValueError("alpha, beta and gamma must be > 0")
    if abs(alpha + beta + gamma - 1.0) >= 1e-9:
        raise ValueError("alpha + beta + gamma must equal 1")
    if delta_in < 0 or delta_out < 0:
        raise ValueError("delta_in and delta_out must be >= 0")
    draws = _Draws(seed)

    def choose(candidates, count, delta):
        if delta > 0:
            bias = count * delta
            if draws.random() < bias / (bias + len(candidates)):
                return draws.below(count)          # node_list is 0 .. count-1
        return draws.choice(candidates)

    vs, ws = [0, 1, 2], [1, 2, 0]      # tails and heads of all arcs: out- and in-degree multisets
    count = 3
    while count < n:
        r = draws.random()
        if r < alpha:
            v = count
            count += 1
            w = choose(ws, count, delta_in)
        elif r < alpha + beta:
            v = choose(vs, count, delta_out)
            w = choose(ws, count, delta_in)
        else:
            v = choose(vs, count, delta_out)
            w = count
            count += 1
        vs.append(v)
        ws.append(w)
    edges = _canonical(count, vs, ws)
    return (edges, count) if return_vertices else edges


def generate_scale_free(n=100, alpha=0.41, beta=0.54, gamma=0.05, delta_in=0.2, delta_out=0, seed=0):
    """Same signature as the reference's generate_scale_free (generators.py:255-277).  The reference's matrix comes from
    a multigraph, so an entry there can be a multiplicity above 1; this one holds ones (the embedder reads only which
    entries with row < col are non-zero, so the layout input is the same)."""
    edges, count = scale_free_edges(n, alpha, beta, gamma, delta_in, delta_out, seed, return_vertices=True)
    return edges_to_adjacency(count, edges)


def relaxed_caveman_edges(l, k, p, seed=0):
    """networkx.relaxed_caveman_graph as a process: the caveman graph, then every edge (u, v), met while walking the
    vertices in order and the neighbours u has when the walk reaches it, is with probability p rewired to (u, x), x uniform over all vertices,
    unless (u, x) is already there.  networkx can rewire onto the edge's own endpoint (x == u), which leaves a self-loop
    in its graph; the loop is dropped here."""
    _check_probability(p)
    n = l * k
    draws = _Draws(seed)
    adj = [dict() for _ in range(n)]          # insertion-ordered, like networkx's
    for c in range(l):
        for a in range(c * k, c * k + k):
            for b in range(a + 1, c * k + k):
                adj[a][b] = None
                adj[b][a] = None
    seen = set()
    for u in range(n):
        for v in list(adj[u]):          # networkx's edge view walks a copy of u's neighbours too
            if v in seen:
                continue
            if draws.random() < p:
                x = draws.below(n)
                if x in adj[u]:
                    continue
                del adj[u][v]
                if v != u:
                    del adj[v][u]
                adj[u][x] = None
                adj[x][u] = None
        seen.add(u)
    us = [u for u in range(n) for _ in adj[u]]
    vs = [v for u in range(n) for v in adj[u]]
    return _canonical(n, us, vs)


def generate_relaxed_caveman(l=10, k=10, p=0.1, seed=0):
    """Same signature as the reference's generate_relaxed_caveman (generators.py:320-341).  The reference's matrix can
    carry a diagonal entry (networkx rewires an edge onto its own endpoint when x == u); this one has an empty diagonal
    (the embedder reads only the entries with row < col, so the layout input is the same)."""
    return edges_to_adjacency(l * k, relaxed_caveman_edges(l, k, p, seed))
