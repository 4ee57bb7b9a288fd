"""One layout iteration of the reference, stated plainly in numpy at extended precision: what the float64 engine
(csrc/f64.hip) is compared with.  TEST INFRASTRUCTURE ONLY.  Written from the description of the reference's iteration
(graphem_rapids/backends/embedder_pytorch.py, "pt.py" below), as oracle/torch_cpu.py is -- not copied.

All arithmetic runs in np.longdouble (x87 80-bit: eps 1.08e-19) and results come back as long double, so against a float64
implementation this module's own rounding is invisible.  Where long double is no wider than that (eps >= 2e-19: it is an
alias of double on some platforms) the module computes in float64 and says so once; the callers' bars do not move.

Neighbour rows and sample ids are integers: knn_rows is a float64 brute force (the engine's rows are defined on double
distances), sample_ids an integer-only restatement of the device sampler documented in csrc/common.h.
"""
import numpy as np

LD = np.longdouble
if not np.finfo(np.longdouble).eps < 2e-19:
    LD = np.float64
    print("f64_reference: np.longdouble is not an extended type here (eps %g): computing in float64"
          % np.finfo(np.longdouble).eps)


def _ld(a):
    return np.asarray(a, dtype=LD)


def scatter_add(n, idx, vals):
    """out[idx[r]] += vals[r] for every row r (index_add_), as one sorted segment sum: out is (n, D) long double."""
    out = np.zeros((n, vals.shape[1]), dtype=LD)
    if len(idx) == 0:
        return out
    order = np.argsort(idx, kind="stable")
    sidx = np.asarray(idx)[order]
    starts = np.flatnonzero(np.r_[True, sidx[1:] != sidx[:-1]])
    out[sidx[starts]] = np.add.reduceat(vals[order], starts, axis=0)
    return out


def _norm(diff):
    return np.sqrt((diff * diff).sum(axis=1, keepdims=True))


def spring_forces(pos, edges, L_min=1.0, k_attr=0.2):
    """pt.py:618-634: diff = p2 - p1, dist = |diff| + 1e-6, f = -k_attr (dist - L_min) diff / dist, +f on the first
    endpoint and -f on the second.  (A zero-length edge gives 0 / 1e-6 = 0, not NaN.)"""
    pos, edges = _ld(pos), np.asarray(edges, dtype=np.int64)
    diff = pos[edges[:, 1]] - pos[edges[:, 0]]
    dist = _norm(diff) + LD(1e-6)
    f = (-LD(k_attr) * (dist - LD(L_min))) * (diff / dist)
    return scatter_add(len(pos), np.concatenate([edges[:, 0], edges[:, 1]]), np.concatenate([f, -f]))


def midpoints(pos, edges):
    """pt.py:785."""
    pos, edges = _ld(pos), np.asarray(edges, dtype=np.int64)
    return (pos[edges[:, 0]] + pos[edges[:, 1]]) / LD(2.0)


def _orient(a, b, c):
    """pt.py:760-763: coordinates 0 and 1 only."""
    return (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])


def crossing_pairs(pos, edges, sampled, knn):
    """The (i, j) edge pairs of pt.py:668-719 that receive a force, one entry per LISTED pair (a pair listed twice is
    there twice): i < j (pt.py:672), no shared vertex (pt.py:685-692), strictly opposite orientations (pt.py:772)."""
    pos, edges = _ld(pos), np.asarray(edges, dtype=np.int64)
    knn = np.asarray(knn, dtype=np.int64)
    i = np.repeat(np.asarray(sampled, dtype=np.int64), knn.shape[1])
    j = knn.reshape(-1)
    keep = i < j
    i, j = i[keep], j[keep]
    e1, e2 = edges[i], edges[j]
    share = (e1[:, 0] == e2[:, 0]) | (e1[:, 0] == e2[:, 1]) | (e1[:, 1] == e2[:, 0]) | (e1[:, 1] == e2[:, 1])
    i, j, e1, e2 = i[~share], j[~share], e1[~share], e2[~share]
    p1, p2, q1, q2 = pos[e1[:, 0]], pos[e1[:, 1]], pos[e2[:, 0]], pos[e2[:, 1]]
    hit = (_orient(p1, p2, q1) * _orient(p1, p2, q2) < 0) & (_orient(q1, q2, p1) * _orient(q1, q2, p2) < 0)
    return i[hit], j[hit]


def intersection_forces(pos, edges, sampled, knn, k_inter=0.5):
    """pt.py:668-734 for the given neighbour ids: every crossing pair pushes its four endpoints away from the mean of the
    four, k_inter diff / (|diff| + 1e-6)^2.  With one component there are no forces: the crossing test reads coordinates
    0 and 1 (pt.py:762-763), which a one-component layout does not have -- the engine returns zeros for D < 2 and so does
    this function."""
    pos, edges = _ld(pos), np.asarray(edges, dtype=np.int64)
    n, D = pos.shape
    if D < 2:
        return np.zeros((n, D), dtype=LD)
    i, j = crossing_pairs(pos, edges, sampled, knn)
    e1, e2 = edges[i], edges[j]
    ends = [e1[:, 0], e1[:, 1], e2[:, 0], e2[:, 1]]
    centre = (pos[ends[0]] + pos[ends[1]] + pos[ends[2]] + pos[ends[3]]) / LD(4.0)     # pt.py:722
    vals = []
    for v in ends:                                                                     # pt.py:727-734
        diff = pos[v] - centre
        dist = _norm(diff) + LD(1e-6)
        vals.append(LD(k_inter) * diff / (dist * dist))
    return scatter_add(n, np.concatenate(ends), np.concatenate(vals) if len(i) else np.zeros((0, D), dtype=LD))


def update(pos, Fs, Fi):
    """pt.py:796-804: new = pos + (Fs + Fi); subtract the column means; divide by the unbiased std + 1e-6."""
    new = _ld(pos) + (_ld(Fs) + _ld(Fi))
    n = new.shape[0]
    new = new - new.sum(axis=0, keepdims=True) / LD(n)
    std = np.sqrt((new * new).sum(axis=0, keepdims=True) / LD(n - 1)) + LD(1e-6)
    return new / std


def step(pos, edges, sampled=None, knn=None, L_min=1.0, k_attr=0.2, k_inter=0.5):
    """pt.py:776-806 with the neighbour rows given (sampled None or empty: spring forces and update only)."""
    Fs = spring_forces(pos, edges, L_min, k_attr)
    if sampled is None or len(sampled) == 0:
        Fi = np.zeros_like(Fs)
    else:
        Fi = intersection_forces(pos, edges, sampled, knn, k_inter)
    return update(pos, Fs, Fi)


def _row_distances(mid, q):
    d2 = np.zeros(len(mid))
    for d in range(mid.shape[1]):      # coordinate order, as the engine's chain (which fuses the multiply-add)
        diff = mid[q, d] - mid[:, d]
        d2 += diff * diff
    return d2


def _first(d2, m):
    """ids of the m smallest (distance, id) keys, in order."""
    m = min(m, len(d2))
    bound = np.partition(d2, m - 1)[m - 1]
    cand = np.flatnonzero(d2 <= bound)
    return cand[np.lexsort((cand, d2[cand]))][:m]


def knn_rows(mid, sampled, k):
    """pt.py:381-424: the k + 1 nearest midpoints of every sampled one, column 0 dropped (pt.py:421).  Brute force in
    float64 over all midpoints, ties on the smaller id."""
    mid = np.asarray(mid, dtype=np.float64)
    return np.stack([_first(_row_distances(mid, q), k + 1)[1:] for q in sampled]).astype(np.int32)


def knn_gap(mid, sampled, k):
    """The smallest relative gap (d[r + 1] - d[r]) / d[r + 1] between consecutive squared distances among the first k + 2
    of any row: how far the rows are from hinging on the last bits of a distance."""
    mid = np.asarray(mid, dtype=np.float64)
    worst = np.inf
    for q in sampled:
        d2 = _row_distances(mid, q)
        d = d2[_first(d2, k + 2)]
        with np.errstate(divide="ignore", invalid="ignore"):
            gap = np.where(d[1:] > 0, (d[1:] - d[:-1]) / d[1:], 0.0)
        worst = min(worst, float(gap.min()))
    return worst


_M64 = (1 << 64) - 1


def _mix32(x):
    """gh_mix32 (csrc/common.h): the 64-bit finaliser, low 32 bits."""
    x &= _M64
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & _M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & _M64
    x ^= x >> 33
    return x & 0xFFFFFFFF


def sample_ids(E, S, seed, iteration):
    """gh_sample_id (csrc/common.h) for t = 0 .. S - 1: the t-th value of a keyed permutation of [0, E) -- a 4-round
    Feistel network on ceil(log2 E) bits (at least one), the halves modified alternately, cycle walking until the value is
    below E.  Python integers only."""
    bits = 1
    while (1 << bits) < E:
        bits += 1
    lb = bits // 2
    hb = bits - lb
    lmask, hmask = (1 << lb) - 1, (1 << hb) - 1
    key = (seed * 0x9E3779B97F4A7C15 + iteration * 0xD1B54A32D192ED03 + 0x2545F4914F6CDD1D) & _M64
    out = np.empty(S, dtype=np.int32)
    for t in range(S):
        x = t
        while True:
            lo, hi = x & lmask, (x >> lb) & hmask
            for rnd in range(4):
                if rnd % 2 == 0:
                    hi = (hi ^ _mix32(key + (rnd << 56) + lo)) & hmask
                else:
                    lo = (lo ^ _mix32(key + (rnd << 56) + hi)) & lmask
            x = (hi << lb) | lo
            if x < E:
                break
        out[t] = x
    return out


# ---- inputs shared by the CPU anchor and the GPU tests -------------------------------------------------------------

LADDER_DEGREES = (1, 2, 3, 4, 5, 7, 8, 9, 12)
LADDER_RUN = 1400          # vertices per run (even, more than twice the largest degree)
LADDER_ISOLATED = 1000
LADDER_HUBS = (1000, 5000)


def degree_ladder(seed=0):
    """(n, edges): 1000 isolated vertices; for each degree of LADDER_DEGREES a run of 1400 vertices of exactly that degree
    (a circulant: offsets 1 .. d // 2, plus the antipodal matching when d is odd); one vertex of degree 1000 and one of
    5000, each on leaves of its own.  The edge list is shuffled and every edge's endpoints are swapped at random."""
    rng = np.random.default_rng(seed)
    parts, base = [], LADDER_ISOLATED
    for d in LADDER_DEGREES:
        m = LADDER_RUN
        v = np.arange(m)
        for off in range(1, d // 2 + 1):
            parts.append(np.stack([base + v, base + (v + off) % m], axis=1))
        if d % 2:
            parts.append(np.stack([base + v[: m // 2], base + v[: m // 2] + m // 2], axis=1))
        base += m
    for d in LADDER_HUBS:
        parts.append(np.stack([np.full(d, base), base + 1 + np.arange(d)], axis=1))
        base += d + 1
    edges = np.concatenate(parts)
    edges = edges[rng.permutation(len(edges))]
    swap = rng.random(len(edges)) < 0.5
    edges[swap] = edges[swap][:, ::-1]
    return base, np.ascontiguousarray(edges, dtype=np.int32)


PLANTED_K = 32
PLANTED_COUNTS = dict(listed=59 * 32, crossing=8 * 32 + 30 * 21, i_gt_j=30 * 8 + 21 * 32, touching=30, collinear=30,
                      shared=30, hub=8 * 32)


def planted_intersections(D, seed=0):
    """(pos, edges, sampled, knn, hub): a layout whose crossings are known.  Coordinates 0 and 1 are integers of at most 64
    in size -- every orientation product is exact in double -- the others Gaussian.
      fans       8 edges from one hub vertex (-64, 0) to (64, y): ids 0..7
      verticals  30 edges x = const from y = -64 to 64: ids 8..37; every fan crosses every vertical properly
      horizontals 21 edges y = const from x = -63 to 63: ids 38..58; each crosses every vertical properly
      touching   per vertical an edge that starts ON it (an endpoint of one on the other segment): ids 59..88
      collinear  per vertical an edge lying on it, overlapping: ids 89..118
      shared     per vertical an edge from its upper endpoint across the horizontals' region: ids 119..148
    Rows (k = 32): a fan lists every vertical and two of them twice (256 crossing pairs, all with the hub as an endpoint,
    a pair listed twice counts twice); a vertical lists the 8 fans (i > j: no force; these are the fans' pairs from the other
    side), the 21 horizontals (crossing), its touching, collinear and shared-vertex edge; a horizontal lists the 30
    verticals and two fans (all i > j).  Edge endpoints are swapped at random."""
    rng = np.random.default_rng(seed + 1000 * D)
    xy, edges = [], []

    def vertex(x, y):
        xy.append((x, y))
        return len(xy) - 1

    hub = vertex(-64, 0)
    for f in range(8):
        edges.append((hub, vertex(64, -56 + 16 * f)))
    vx = [-60 + 4 * b for b in range(30)]
    tops = []
    for x in vx:
        lo, hi = vertex(x, -64), vertex(x, 64)
        tops.append(hi)
        edges.append((lo, hi))
    for a in range(21):
        edges.append((vertex(-63, -60 + 6 * a), vertex(63, -60 + 6 * a)))
    for x in vx:
        edges.append((vertex(x, 10), vertex(x + 2, 13)))
    for x in vx:
        edges.append((vertex(x, -10), vertex(x, 30)))
    for b, x in enumerate(vx):
        edges.append((tops[b], vertex(x + 1, -64)))
    n = len(xy) + 7                                     # a few vertices no edge touches
    edges = np.array(edges, dtype=np.int64)
    swap = rng.random(len(edges)) < 0.5
    edges[swap] = edges[swap][:, ::-1]
    pos = rng.standard_normal((n, D))
    m = min(D, 2)
    pos[:, :m] = 0.0
    pos[: len(xy), :m] = np.array(xy, dtype=np.float64)[:, :m]
    fans, vert, hor = np.arange(8), 8 + np.arange(30), 38 + np.arange(21)
    rows = [np.concatenate([vert, vert[[f, (f + 7) % 30]]]) for f in fans]
    rows += [np.concatenate([fans, hor, [59 + b, 89 + b, 119 + b]]) for b in range(30)]
    rows += [np.concatenate([vert, fans[[a % 8, (a + 3) % 8]]]) for a in range(21)]
    sampled = np.concatenate([fans, vert, hor]).astype(np.int32)
    return pos, np.ascontiguousarray(edges, dtype=np.int32), sampled, np.stack(rows).astype(np.int32), hub


def classify_planted(pos, edges, sampled, knn, hub):
    """Counts of every kind of listed pair, from exact integer arithmetic on coordinates 0 and 1 (Python ints): the truth
    the planted layout is checked against, independent of the floating-point functions above."""
    P = [(int(x), int(y)) for x, y in np.asarray(pos)[:, :2]]
    assert np.array_equal(np.asarray(pos)[:, :2], np.array(P, dtype=np.float64))

    def orient(a, b, c):
        return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])

    def between(a, b, c):       # c on the closed segment a-b, given that it is collinear with it
        return min(a[0], b[0]) <= c[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= c[1] <= max(a[1], b[1])

    out = dict(listed=0, crossing=0, i_gt_j=0, touching=0, collinear=0, shared=0, hub=0)
    for i, row in zip(sampled, knn):
        for j in row:
            out["listed"] += 1
            if not i < j:
                out["i_gt_j"] += 1
                continue
            a, b, c, d = (int(v) for v in (*edges[i], *edges[j]))
            if len({a, b, c, d}) < 4:
                out["shared"] += 1
                continue
            o = [orient(P[a], P[b], P[c]), orient(P[a], P[b], P[d]), orient(P[c], P[d], P[a]), orient(P[c], P[d], P[b])]
            if o[0] * o[1] < 0 and o[2] * o[3] < 0:
                out["crossing"] += 1
                out["hub"] += hub in (a, b, c, d)
            elif all(v == 0 for v in o):
                assert between(P[a], P[b], P[c]) or between(P[a], P[b], P[d]) or between(P[c], P[d], P[a])
                out["collinear"] += 1
            elif (o[0] == 0 and between(P[a], P[b], P[c])) or (o[1] == 0 and between(P[a], P[b], P[d])) or \
                    (o[2] == 0 and between(P[c], P[d], P[a])) or (o[3] == 0 and between(P[c], P[d], P[b])):
                out["touching"] += 1
    return out
