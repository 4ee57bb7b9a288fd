"""Thresholds from coarse group minima inside the query-cell launch (csrc/setup_core.h "COARSE FORM", csrc/qcell_core.h
gh_ct_tau, spring_scan_cells_kernel<D, KC > 0>) against the fine group minima and the threshold launch they replace, on the
same engine inputs with the query-cell filter forced: tau only decides how many candidates are parked, so the neighbour
rows and a step's positions must be the same bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K_NN = 10
GROUPS = 64          # GH_CT_M
EMPTY = 0xFFFFFFFF   # GH_CT_EMPTY


def _rr(n, deg, seed):
    import graphem_rapids_amd as gra
    return gra.random_regular_edges(n, deg, seed=seed).astype(np.int32)


@pytest.fixture(scope="module")
def rr20k():
    return _rr(20000, 8, 31)   # 80 000 edges: 70 set-up workgroups, every coarse group occupied


def _engine(n, D, edges, S, form, dist="exact", k=K_NN, seed=3):
    from graphem_rapids_amd import _native
    eng = _native.Engine(n, D, edges, 1.0, 0.2, 0.5, k, S, seed=seed, knn_distance=dist)
    eng.set_scan_filter("cells")
    eng.set_coarse_tau(form)
    assert eng.scan_filter() == "cells"
    assert eng.coarse_tau() == (form == "on")
    return eng


def _rows_and_step(n, D, edges, S, pos, sampled, form, dist="exact", k=K_NN, step=True):
    eng = _engine(n, D, edges, S, form, dist, k)
    eng.set_positions(pos)
    rows = eng.knn_midpoints(sampled)
    out = None
    if step:
        eng.set_positions(pos)
        eng.step(sampled)
        out = eng.get_positions()
    counts = eng.knn_last_counts()
    eng.sync()   # (raises if a workgroup gave up waiting for the table: wait_failed)
    eng.close()
    return rows, out, counts


def _same(n, D, edges, S, pos, sampled, dist="exact", k=K_NN, step=True):
    old = _rows_and_step(n, D, edges, S, pos, sampled, "off", dist, k, step)
    new = _rows_and_step(n, D, edges, S, pos, sampled, "on", dist, k, step)
    assert np.array_equal(old[0], new[0])
    if step:
        assert old[1].tobytes() == new[1].tobytes()
    return old, new


@pytest.mark.parametrize("D,S", [(3, 256), (3, 1), (3, 255), (2, 256)])
def test_rows_and_one_step_match_the_threshold_launch(D, S, rr20k):
    n = 20000
    rng = np.random.default_rng(10 * D + S)
    pos = (rng.standard_normal((n, D)) * 0.1).astype(np.float32)
    sampled = rng.permutation(len(rr20k))[:S].astype(np.int32)
    old, new = _same(n, D, rr20k, S, pos, sampled)
    assert not np.asarray(new[2][2]).any()   # no candidate list overflowed: the rows came through the filtered scan


@pytest.mark.parametrize("dist,k", [("cdist", K_NN), ("exact", 20), ("exact", 31)])
def test_more_keys_than_neighbours(dist, k, rr20k):
    """Parity mode bounds K + 1 keys; more than 12 keys take the kernel with 32 registers per thread (31 neighbours: all)."""
    n = 20000
    rng = np.random.default_rng(k)
    pos = (rng.standard_normal((n, 3)) * 0.1).astype(np.float32)
    sampled = rng.permutation(len(rr20k))[:256].astype(np.int32)
    _same(n, 3, rr20k, 256, pos, sampled, dist=dist, k=k)


def test_empty_coarse_groups():
    """24 000 edges: 47 set-up workgroups for 64 groups, 17 of them stay empty."""
    n = 6000
    edges = _rr(n, 8, 5)
    rng = np.random.default_rng(1)
    pos = (rng.standard_normal((n, 3)) * 0.1).astype(np.float32)
    sampled = rng.permutation(len(edges))[:256].astype(np.int32)
    _same(n, 3, edges, 256, pos, sampled)
    eng = _engine(n, 3, edges, 256, "on")
    eng.set_positions(pos)
    eng.step()                       # own ids: its normalise launch has set the next iteration up
    tab = eng.coarse_table()
    eng.close()
    filled = (tab != EMPTY).any(axis=2)          # (copy, group)
    assert filled[1].sum() == 47 and not filled[0].any()
    assert (tab[1][filled[1]] <= 0x7F800000).all()


def test_fewer_than_k_reachable_groups(rr20k):
    """All but a few vertices at +inf: fewer than K groups hold a finite minimum, tau = +inf, every query goes on the wide
    list and through the exact fallback -- the same rows as with the threshold launch."""
    n = 20000
    rng = np.random.default_rng(2)
    S = 33
    sampled = rng.permutation(len(rr20k))[:S].astype(np.int32)
    pos = np.full((n, 3), np.inf, dtype=np.float32)
    keep = np.unique(rr20k[sampled[:5]])                      # five finite queries; at most a few more finite midpoints
    pos[keep] = (rng.standard_normal((len(keep), 3)) * 0.1).astype(np.float32)
    finite_mid = np.isfinite(pos[rr20k].sum(axis=(1, 2))).sum()
    assert 5 <= finite_mid < K_NN + 1
    old, new = _same(n, 3, rr20k, S, pos, sampled, step=False)
    assert np.asarray(new[2][2])[:5].all()                    # exact fallback


def test_coincident_positions():
    """2000 vertices on 16 distinct points: thousands of midpoints coincide to the bit (copies count in the selection)."""
    n = 2000
    edges = _rr(n, 20, 9)   # 20 000 edges: enough for the filtered scan
    rng = np.random.default_rng(3)
    spots = (rng.standard_normal((16, 3)) * 0.1).astype(np.float32)
    pos = spots[rng.integers(0, 16, size=n)]
    sampled = rng.permutation(len(edges))[:256].astype(np.int32)
    _same(n, 3, edges, 256, pos, sampled)


def test_consecutive_steps_use_and_reset_both_copies(rr20k):
    n, D, S = 20000, 3, 256
    rng = np.random.default_rng(4)
    pos = (rng.standard_normal((n, D)) * 0.1).astype(np.float32)
    given = rng.permutation(len(rr20k))[:S].astype(np.int32)
    out, tabs = {}, {}
    for form in ("off", "on"):
        eng = _engine(n, D, rr20k, S, form, seed=17)
        eng.set_positions(pos)
        after = []
        for _ in range(3):               # the engine's own ids: every normalise launch sets the next iteration up
            eng.step()
            after.append(eng.get_positions())
        if form == "on":
            tabs[3] = eng.coarse_table()
        eng.step(given)                  # ids from the host: the set-up done ahead is stale, the stand-alone kernel runs
        after.append(eng.get_positions())
        if form == "on":
            tabs[4] = eng.coarse_table()
        eng.sync()
        eng.close()
        out[form] = after
    for a, b in zip(out["off"], out["on"]):
        assert a.tobytes() == b.tobytes()
    assert tabs[3].shape == (2, GROUPS, S)
    # after iteration 3 (iterations 0..2 done): the set-up of iteration 3 has filled copy 1, copy 0 is empty again
    assert (tabs[3][0] == EMPTY).all()
    assert (tabs[3][1] <= 0x7F800000).all()
    # after the step with given ids nothing is set up ahead: that copy was refilled and consumed, both are empty
    assert (tabs[4] == EMPTY).all()


def test_switch_reports_what_is_in_use(rr20k):
    from graphem_rapids_amd import _native
    eng = _native.Engine(20000, 3, rr20k, 1.0, 0.2, 0.5, K_NN, 256)
    assert eng.scan_filter() == "mfma" and not eng.coarse_tau()   # thresholds embedded in the fused launch: neither
    eng.set_scan_filter("cells")
    on = eng.coarse_tau()
    assert on                        # AUTO: three components, 11 keys
    eng.set_coarse_tau("off")
    assert not eng.coarse_tau()
    eng.set_coarse_tau("on")
    assert eng.coarse_tau()
    eng.set_coarse_tau("auto")
    assert eng.coarse_tau() == on
    eng.close()
    eng = _native.Engine(20000, 3, rr20k, 1.0, 0.2, 0.5, 40, 256)   # 41 keys: more than the selection holds
    eng.set_scan_filter("cells")
    eng.set_coarse_tau("on")
    assert not eng.coarse_tau()
    eng.close()
