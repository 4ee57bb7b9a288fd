"""The cascade and RR-set launches of influence.hip and ris.hip past their grid caps: the shapes A - E of
tests/launch_caps.py, the smallest at which ic_pull_kernel, ic_advance_kernel, ic_count_kernel, ic_reset_kernel,
ic_push_kernel, rr_scatter_kernel and the coverage kernels take a second trip of their loop.  The other GPU tests of these
files stay an order of magnitude below.  tests/test_launch_caps_cpu.py holds, by the restatements, that each shape still
sends more than a trip through the kernel its row names.

Everything is compared bit for bit with the numpy restatements (tests/ic_reference.py, arc_ic_reference.py,
ris_reference.py), computed once in tests/cascade_caps.py.  In the order A - E: the cheapest shows a fault first."""
import numpy as np
import pytest

from graphem_rapids_amd import _native

import cascade_caps as cc
import launch_caps as lc
import ris_reference as ris

pytestmark = pytest.mark.gpu

KINDS = ["p", "arcs"]   # the scalar threshold, and the ARC instantiations over a table with exact 0 and 1 mixed in


def _ic_graph(n, pairs, directed, prob, kind):
    g = _native.ICGraph(n, pairs, directed)
    if kind == "arcs":
        if directed:
            g.set_arc_probabilities(pairs, prob)
        else:
            g.set_arc_probabilities(*cc.arc.as_directed(pairs, False, prob))
    return g


def _same_collection(rr, want):
    indptr, members, roots = rr.download()
    assert rr.counts() == (len(want[2]), len(want[1]))
    assert np.array_equal(roots, want[2])
    assert np.array_equal(indptr, want[0])
    assert np.array_equal(members, want[1])


# ---- A -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_forward_pull_past_the_cap(kind):
    """17 seed sets on er2000, 1000 trials: 17 * 2003 * 16 = 544 816 words of dense state against 524 288 a trip, the last
    set across the boundary.  The frontier passes pull_min = 2128 entries from the third level on (17 970, 33 435, 33 915,
    ...), so ic_pull_kernel scans the dense state, and ic_advance_kernel, ic_count_kernel and ic_reset_kernel walk some
    34 000 entries of 16 words; the first two levels and the tail push."""
    s = lc.FWD_PULL
    n, pairs, sets, prob = cc.forward_pull()
    want, _, _ = cc.forward_pull_expected(kind == "arcs")
    g = _ic_graph(n, pairs, False, prob, kind)
    totals, got = g.spread(sets, None if kind == "arcs" else s["p"], s["T"], cc.IC_SEED, -1, per_trial=True)
    again = g.spread(sets[-2:], None if kind == "arcs" else s["p"], s["T"], cc.IC_SEED, -1, per_trial=True)[1]
    g.close()
    assert got.shape == (s["sets"], s["T"]) and got.dtype == np.int32
    for j, (row, need) in enumerate(zip(got, want)):
        assert np.array_equal(row, need), f"set {j}"
    assert np.array_equal(totals, want.sum(axis=1))
    assert np.array_equal(again, want[-2:])   # ic_reset_kernel left the state zero, past its first trip too


# ---- B -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_forward_push_past_the_cap(kind):
    """8 sets of 1060 seeds, 4033 trials (64 words, one valid bit in the last), one hop: 8480 frontier entries stay under
    pull_min = 8751, and 8480 * 64 = 542 720 (entry, word) items pass the 524 288 of a trip of ic_push_kernel; the second
    trip holds entries of the last set only."""
    s = lc.FWD_PUSH
    n, pairs, sets, prob = cc.forward_push()
    want = cc.forward_push_expected(kind == "arcs")
    g = _ic_graph(n, pairs, True, prob, kind)
    totals, got = g.spread(sets, None if kind == "arcs" else s["p"], s["T"], cc.IC_SEED, 1, per_trial=True)
    g.close()
    for j, (row, need) in enumerate(zip(got, want)):
        assert np.array_equal(row, need), f"set {j}"
    assert np.array_equal(totals, want.sum(axis=1)) and want.min() > s["set_size"]


# ---- C -------------------------------------------------------------------------------------------------------------------
def test_reverse_pull_past_the_cap():
    """1250 samples on a 6-regular graph of 40 003 vertices, p = 0.4, five hops: a chunk of 1216 samples at 19 words, whose
    frontier passes n / 16 = 2500 entries in its second level, so ic_pull_kernel<REV> scans 40 003 * 19 = 760 057 words, and
    whose 35 970 touched entries times 19 words pass a trip of ic_count_kernel, rr_scatter_kernel and ic_reset_kernel; then
    a chunk of 34 samples at one word.  Coverage and hit counts on the collection afterwards."""
    s = lc.REV_PULL
    n, pairs = cc.reverse_pull()
    want, _ = cc.reverse_pull_expected()
    g = _native.ICGraph(n, pairs, False)
    rr = _native.RRSets(n)
    g.rr_sample(rr, s["samples"], s["p"], cc.IC_SEED, s["hops"])
    _same_collection(rr, want)
    seeds, gains = rr.cover(10)
    want_seeds, want_gains = ris.max_coverage(want[0], want[1], n, 10)
    assert seeds.tolist() == want_seeds and np.array_equal(gains, want_gains)
    for verts in ([], [0], [n - 1, n - 2], list(range(0, n, 7)), want_seeds):
        assert rr.count_hit(verts) == ris.count_hit(want[0], want[1], verts)
    rr.close()
    rr = _native.RRSets(n)   # the same draw again: the chunk state was left zero
    g.rr_sample(rr, 64, s["p"], cc.IC_SEED, s["hops"])
    got = rr.download()
    assert np.array_equal(got[0], want[0][:65]) and np.array_equal(got[1], want[1][:want[0][64]])
    rr.close()
    g.close()


# ---- D -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_reverse_push_past_the_cap(kind):
    """8192 samples in one chunk of 128 words on 262 147 vertices, explicit trials, 8000 distinct roots (rr_root_kernel sees
    shared ones), one hop: 8000 entries stay under n / 16 = 16 384 and make 1 024 000 (entry, word) items, two trips of
    ic_push_kernel<REV>, the second a partial one."""
    s = lc.REV_PUSH
    n, pairs, trials, roots, prob = cc.reverse_push()
    want = cc.reverse_push_expected(kind == "arcs")
    g = _ic_graph(n, pairs, True, prob, kind)
    rr = _native.RRSets(n)
    g.rr_sample(rr, s["samples"], None if kind == "arcs" else s["p"], cc.IC_SEED, 1, trials=trials, roots=roots)
    _same_collection(rr, want)
    rr.close()
    g.close()
    assert np.diff(want[0]).max() == s["in_degree"] + 1 and np.diff(want[0]).min() == 1


# ---- E -------------------------------------------------------------------------------------------------------------------
def test_coverage_kernels_past_their_caps():
    """9003 uploaded sets over 300 001 vertices, 514 140 members: rr_vscatter_kernel and rr_hit_kernel take 4096 sets a trip,
    rr_argmax_kernel 262 144 vertices, rr_vcount_kernel 262 144 members, and rr_cover_kernel 1024 sets of the chosen vertex
    -- vertex 290 000, above the first argmax trip, is in 3001.  Then vertices 1234 and 280 000 lead with 40 sets each, one
    on each trip of the argmax: the smaller id wins."""
    e = lc.COVER
    n, indptr, members = cc.cover_system()
    rr = _native.RRSets(n)
    rr.upload(indptr, members)
    for k in (1, 12):
        seeds, gains = rr.cover(k)
        want_seeds, want_gains = cc.cover_expected(k)
        assert seeds.tolist() == want_seeds and np.array_equal(gains, want_gains), k
    assert want_seeds[:3] == [e["heavy"], e["tie_low"], e["tie_high"]]
    for verts in ([], [e["heavy"]], list(range(0, n, 7)), want_seeds):
        assert rr.count_hit(verts) == ris.count_hit(indptr, members, verts)
    got = rr.download()
    assert np.array_equal(got[0], indptr) and np.array_equal(got[1], members) and (got[2] == -1).all()
    rr.close()
