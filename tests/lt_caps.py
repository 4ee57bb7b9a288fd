"""The shapes at which tests/test_hip_lt_influence.py takes the Linear Threshold launches of influence.hip (lt_push_kernel,
lt_pull_kernel, forward and reverse) past IC_MAX_BLOCKS workgroups, and what tests/lt_reference.py gives for them, each
computed once per process.  The graphs, seed sets and samples are those of tests/cascade_caps.py (shapes A, B and D of
tests/launch_caps.py) under uniform weights; tests/test_lt_influence_cpu.py holds, by the restatement and the sizing rules
as the sources state them, that each still sends more than a trip through the launch it is meant for.

Reverse pull has no such shape, by the sizing rules themselves: an RR set under Linear Threshold is a path, so a level's
frontier has at most one entry per sample of the chunk, 64 W, and gh_ic_rr_sample takes W <= max(RR_MIN_WORDS_CAP,
n / (128 IC_PULL_DIV)) words.  A level pulls from n / IC_PULL_DIV entries on, so it can pull only while
64 RR_MIN_WORDS_CAP >= n / IC_PULL_DIV, and then the dense state n W is at most 64 IC_PULL_DIV RR_MIN_WORDS_CAP^2 words:
reverse_pull_reach() evaluates both sides.  REV_PULL is the largest-state shape that pulls at all."""
import functools

import numpy as np

import graphem_rapids_amd as gr

import cascade_caps as cc
import ic_reference as ic
import launch_caps as lc
import lt_reference as lt

IC_SEED = cc.IC_SEED
REV_PULL = dict(n=16_003, degree=6, samples=1024, hops=3)


def _uniform(n, pairs, directed):
    return gr.lt_weights(pairs, n, directed, "uniform")


def _filtered(rows, keep):
    return tuple(x[keep] for x in rows)


# ---- forward pull: shape A -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def forward_pull():
    """(n, canonical pairs, seed sets, (A, 2) uniform weights)."""
    n, pairs, sets, _ = cc.forward_pull()
    return n, pairs, sets, _uniform(n, pairs, False)


@functools.lru_cache(maxsize=None)
def forward_pull_expected():
    """((sets, T) int64 counts, frontier entries of the chunk per level, touched entries of the chunk)."""
    s = lc.FWD_PULL
    n, pairs, sets, weight = forward_pull()
    rows, fronts = [], []
    for seeds in sets:
        f = ic.Frontiers()
        rows.append(lt.spread_trials_lt(n, pairs, False, weight, seeds, s["T"], IC_SEED, None, frontiers=f))
        fronts.append(f)
    depth = max(len(f.entries()) for f in fronts)
    entries = [sum(f.entries()[r] for f in fronts if r < len(f.entries())) for r in range(depth)]
    return np.array(rows), entries, sum(f.touched_entries() for f in fronts)


# ---- forward push: shape B -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def forward_push():
    """(n, canonical pairs, seed sets, (A,) uniform weights)."""
    n, pairs, sets, _ = cc.forward_push()
    return n, pairs, sets, _uniform(n, pairs, True)


@functools.lru_cache(maxsize=None)
def forward_push_expected():
    """(sets, T) int64 counts after one hop.  The intervals are those of the whole graph; of them the restatement of a set
    gets the arcs that leave a seed, since no other arc can carry anything in one hop."""
    s = lc.FWD_PUSH
    n, pairs, sets, weight = forward_push()
    rows = lt.rows_of(n, pairs, True, weight)
    return np.array([lt.spread_trials_lt(n, None, True, None, seeds, s["T"], IC_SEED, 1, rows=_filtered(rows, np.isin(rows[0], seeds)))
                     for seeds in sets])


# ---- reverse push: shape D -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reverse_push():
    """(n, canonical pairs, trials, roots, (A,) uniform weights)."""
    n, pairs, trials, roots, _ = cc.reverse_push()
    return n, pairs, trials, roots, _uniform(n, pairs, True)


@functools.lru_cache(maxsize=None)
def reverse_push_expected():
    """(indptr, members, roots) after one hop, from the arcs whose head is a root: no other arc is walked."""
    n, pairs, trials, roots, weight = reverse_push()
    rows = lt.rows_of(n, pairs, True, weight)
    return lt.rr_sets_lt(n, None, True, None, seed=IC_SEED, max_hops=1, trials=trials, roots=roots,
                         rows=_filtered(rows, np.isin(rows[1], roots)))


# ---- reverse pull: below the cap -----------------------------------------------------------------------------------------
def reverse_pull_reach(d):
    """(largest n at which a reverse level can pull, words per chunk there, dense words there): the bound of the module
    docstring from the defines."""
    n_max = 64 * d.RR_MIN_WORDS_CAP * d.IC_PULL_DIV + d.IC_PULL_DIV - 1
    W = lc.rr_words_per_chunk(d, n_max, 64 * d.RR_MAX_WORDS)
    return n_max, W, n_max * W


@functools.lru_cache(maxsize=None)
def reverse_pull():
    """(n, canonical pairs, roots, (A, 2) uniform weights): 1024 distinct roots, so round 1's frontier has 1024 entries."""
    s = REV_PULL
    n = s["n"]
    pairs = ic.canonical_arcs(n, gr.random_regular_edges(n - 3, s["degree"], seed=3), False)
    roots = np.random.default_rng(37).choice(n - 3, s["samples"], replace=False)
    return n, pairs, roots, _uniform(n, pairs, False)


@functools.lru_cache(maxsize=None)
def reverse_pull_expected():
    """((indptr, members, roots), Frontiers)."""
    s = REV_PULL
    n, pairs, roots, weight = reverse_pull()
    f = ic.Frontiers(lc.rr_words_per_chunk(lc.defines(), n, s["samples"]))
    return lt.rr_sets_lt(n, pairs, False, weight, s["samples"], IC_SEED, s["hops"], roots=roots, frontiers=f), f
