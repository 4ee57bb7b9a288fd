"""The coarse form of the threshold group minima (csrc/setup_core.h "COARSE FORM", csrc/qcell_core.h gh_ct_tau), restated
in numpy: set-up workgroup b of n takes 128 consecutive subset edges, reduces each query's distances to them to one
minimum and folds it into group b * M // n with an unsigned min on the float bits; tau of a query is the K-th smallest of
its M group minima as a multiset, +inf when fewer than K groups hold anything.  No GPU needed.

tau has to be an upper bound of the query's K-th smallest distance: K different groups with a minimum <= tau hold K
different edges within tau.  How loose it is decides only how many candidates the scan parks: the K-th smallest of M group
minima has expected subset rank r(M) = ln(1 - K/M) / ln(1 - 1/M)."""
import numpy as np
import pytest

TILE = 128                      # GH_THR_TILE: subset edges per set-up workgroup
EMPTY = np.uint32(0xFFFFFFFF)   # GH_CT_EMPTY
INF_BITS = np.uint32(0x7F800000)


def d2_f32(q, m):
    """(Q, D) x (E, D) -> (Q, E) squared distances, accumulated in float32 in coordinate order."""
    out = np.zeros((len(q), len(m)), dtype=np.float32)
    for d in range(q.shape[1]):
        df = q[:, d:d + 1] - m[None, :, d]
        out = (df * df + out).astype(np.float32)
    return out


def coarse_table(d2, M):
    """(Q, M1) distances to the subset edges -> (Q, M) float bits, EMPTY where no workgroup wrote."""
    Q, M1 = d2.shape
    tiles = (M1 + TILE - 1) // TILE
    tab = np.full((Q, M), EMPTY, dtype=np.uint32)
    for b in range(tiles):
        best = np.minimum(d2[:, b * TILE:(b + 1) * TILE].min(axis=1).view(np.uint32), INF_BITS)   # (starts from +inf)
        g = b * M // tiles
        tab[:, g] = np.minimum(tab[:, g], best)
    return tab


def kth_of_multiset(tab, K):
    """K-th smallest entry of every row, copies counted; anything >= +inf (empty entries included) is +inf."""
    kth = np.sort(tab, axis=1)[:, K - 1] if K <= tab.shape[1] else np.full(len(tab), INF_BITS, dtype=np.uint32)
    return np.minimum(kth, INF_BITS).view(np.float32)


def kth_of_distinct(tab, K):
    """What a selection that retires copies WITHOUT counting them would give (the bug gh_tau_kth's comment describes)."""
    out = np.full(len(tab), np.inf, dtype=np.float32)
    for i, row in enumerate(tab):
        u = np.unique(row[row < INF_BITS])
        if len(u) >= K:
            out[i] = u[K - 1:K].view(np.float32)[0]
    return out


def expected_rank(K, M):
    return np.log(1.0 - K / M) / np.log(1.0 - 1.0 / M)


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("K", [2, 11, 33])
@pytest.mark.parametrize("M", [64, 128])
def test_tau_bounds_the_kth_distance(D, K, M):
    rng = np.random.default_rng(100 * D + 10 * K + M)
    E, stride, Q = 40000, 2, 64
    mid = rng.standard_normal((E, D)).astype(np.float32)
    q = mid[rng.permutation(E)[:Q]] + np.float32(0.01) * rng.standard_normal((Q, D)).astype(np.float32)
    d2 = d2_f32(q, mid)
    tau = kth_of_multiset(coarse_table(d2[:, ::stride], M), K)
    assert np.isfinite(tau).all()
    exact = np.sort(d2, axis=1)[:, K - 1]          # over ALL edges, of which the subset is a part
    assert (tau >= exact).all()
    # and it is not vacuous: every query keeps K edges within tau, most of them not many more than K of the subset
    sub_rank = (d2[:, ::stride] <= tau[:, None]).sum(axis=1)
    assert (sub_rank >= K).all() and np.median(sub_rank) <= 2 * K + 2


@pytest.mark.parametrize("M", [64, 128])
def test_copies_are_counted(M):
    """40 midpoints coincide to the bit and are the nearest to the query, one per set-up workgroup of 40 different groups:
    the 11th smallest group minimum is their distance, not the 11th DISTINCT value."""
    rng = np.random.default_rng(M)
    tiles, K = 2 * M, 11
    mid = (rng.standard_normal((tiles * TILE, 3)) + 4.0).astype(np.float32)
    spot = np.array([0.25, -0.5, 0.125], dtype=np.float32)
    owners = np.arange(40) * (tiles // M)              # the first workgroup of 40 different groups
    mid[owners * TILE + rng.integers(0, TILE, size=40)] = spot
    q = np.zeros((1, 3), dtype=np.float32)
    d2 = d2_f32(q, mid)
    tab = coarse_table(d2, M)
    d_spot = d2_f32(q, spot[None, :])[0, 0]
    assert (tab[0] == d_spot.view(np.uint32)).sum() == 40
    assert kth_of_multiset(tab, K)[0] == d_spot
    assert kth_of_distinct(tab, K)[0] > d_spot         # the check above tells the two apart
    assert kth_of_multiset(tab, 40)[0] == d_spot and kth_of_multiset(tab, 41)[0] > d_spot


@pytest.mark.parametrize("M", [64, 128])
@pytest.mark.parametrize("K", [2, 11, 33])
def test_fewer_than_k_occupied_groups_give_inf(M, K):
    rng = np.random.default_rng(7)
    q = rng.standard_normal((5, 2)).astype(np.float32)
    for tiles in (1, K - 1):
        mid = rng.standard_normal((tiles * TILE - 3, 2)).astype(np.float32)   # (the last tile is not full)
        tab = coarse_table(d2_f32(q, mid), M)
        assert ((tab != EMPTY).sum(axis=1) == tiles).all()
        assert np.isposinf(kth_of_multiset(tab, K)).all()
    mid = rng.standard_normal((K * TILE, 2)).astype(np.float32)               # exactly K occupied groups: finite
    assert np.isfinite(kth_of_multiset(coarse_table(d2_f32(q, mid), M), K)).all()
    # a group whose edges are all out of reach (non-finite midpoints) counts as empty
    mid[: 2 * TILE] = np.inf
    assert np.isposinf(kth_of_multiset(coarse_table(d2_f32(q, mid), M), K)).all()


@pytest.mark.parametrize("M", [64, 128])
def test_mean_rank_follows_the_formula(M):
    """r(M) = ln(1 - K/M) / ln(1 - 1/M): 12.0 at M = 64, 11.5 at M = 128 for K = 11 (a check of the formula the choice
    of M rests on, not of the GPU)."""
    K, Q = 11, 2000
    rng = np.random.default_rng(5 + M)
    mid = rng.random((M * TILE, 3), dtype=np.float32)
    ranks = []
    for lo in range(0, Q, 250):
        q = rng.random((250, 3), dtype=np.float32)
        d2 = d2_f32(q, mid)
        tau = kth_of_multiset(coarse_table(d2, M), K)
        ranks.append((d2 <= tau[:, None]).sum(axis=1))
    mean = float(np.concatenate(ranks).mean())
    r = expected_rank(K, M)
    assert abs(r - {64: 12.0, 128: 11.5}[M]) < 0.05
    assert abs(mean - r) <= 0.10 * r, (mean, r)
