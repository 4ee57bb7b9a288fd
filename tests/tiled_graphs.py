"""Expected values on a graph of a million vertices without a slow reference: C disjoint copies of a base graph B of
tests/cores_reference.py (copy c shifted by c n0), all C n0 vertices relabelled by one seeded random permutation, the edge
list shuffled.  The permutation makes the memory layout aperiodic -- no copy is aligned with the stride of a capped launch
-- so a value read from the wrong index is wrong, not accidentally equal.  What the restatements give on B carries over:

  core, onion layer, peel rounds   identical copies peel in lock-step under the global threshold and round counter: every
                                   vertex has B's core and layer, the round count is B's.  Relabelling changes neither.
  truss number, edge-peel rounds   the same; which leaver of a triangle decrements (the one of smaller edge id) does not
                                   change the supports that result.  Listed in the canonical edge order of the tiled graph.
  triangles per vertex             B's value at the vertex's image.
  component labels                 the smallest new id in each (copy, component of B).

tests/test_tiled_graphs_cpu.py runs the restatements on three copies and finds exactly these values.  Nothing here touches
the library under test."""
import functools
import types

import numpy as np

import cores_reference as cref
import graphstats_reference as gsr


@functools.lru_cache(maxsize=None)
def base_values(name):
    """What the restatements give on the base graph, computed once; callers leave the arrays unchanged."""
    _, n0, e0 = cref.graph(name)
    core, layer, rounds = cref.peel_of(name)
    edges, truss, truss_rounds = cref.truss_of(name)
    return types.SimpleNamespace(n=n0, edges=edges, core=core, layer=layer, rounds=rounds, truss=truss, truss_rounds=truss_rounds,
                                 triangles=gsr.triangles(n0, e0), labels=gsr.component_labels(n0, e0))


def tiled(name, copies, seed=0):
    """`copies` relabelled copies of cores_reference graph `name`.  n, edges ((E, 2) int64, shuffled, either endpoint first)
    and perm (the new id of vertex v of copy c is perm[c n0 + v]); the expectations core, layer (int32), rounds, triangles
    (int64), labels (int32) per new vertex id, and canonical (E, 2), truss (int32), truss_rounds in canonical edge order."""
    b = base_values(name)
    n0, C = b.n, int(copies)
    n = C * n0
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n).astype(np.int64)
    old = (b.edges[None, :, :] + (np.arange(C, dtype=np.int64) * n0)[:, None, None]).reshape(-1, 2)   # copy-major, B's canonical order
    new = perm[old]
    lo, hi = new.min(axis=1), new.max(axis=1)
    order = np.argsort(lo * n + hi, kind="stable")   # the key of the canonical order (u < v, ascending)
    flip = rng.random(len(new)) < 0.5
    edges = np.where(flip[:, None], new[:, ::-1], new)[rng.permutation(len(new))]

    def at_image(values):
        out = np.empty(n, dtype=values.dtype)
        out[perm] = np.tile(values, C)
        return out

    group = (np.arange(C, dtype=np.int64) * n0)[:, None] + b.labels[None, :].astype(np.int64)   # (copy, component of B), per old id
    low = np.full(n, n, dtype=np.int64)
    np.minimum.at(low, group.ravel(), perm)
    labels = np.empty(n, dtype=np.int32)
    labels[perm] = low[group.ravel()]
    return types.SimpleNamespace(
        name=name, copies=C, n=n, edges=edges, perm=perm,
        core=at_image(b.core), layer=at_image(b.layer), rounds=b.rounds,
        triangles=at_image(b.triangles), labels=labels,
        canonical=np.column_stack([lo, hi])[order], truss=np.tile(b.truss, C)[order], truss_rounds=b.truss_rounds)
