"""The argument of tests/tiled_graphs.py where the restatements can still run: three relabelled copies of a base graph, and
peel, truss, triangles and component_labels of tests/cores_reference.py and tests/graphstats_reference.py run directly on
the tiled graph.  Their results must equal the helper's expectations exactly."""
import numpy as np
import pytest

import cores_reference as cref
import graphstats_reference as gsr
import tiled_graphs


@pytest.mark.parametrize("name", ["gnp300", "relaxed_caveman", "gnp2000"])
def test_three_copies_equal_the_restatements(name):
    t = tiled_graphs.tiled(name, 3, seed=5)
    b = tiled_graphs.base_values(name)
    assert t.n == 3 * b.n and t.edges.shape == (3 * len(b.edges), 2)
    assert sorted(t.perm.tolist()) == list(range(t.n)) and not np.array_equal(t.perm, np.arange(t.n))
    assert (t.edges[:, 0] > t.edges[:, 1]).any() and (t.edges[:, 0] < t.edges[:, 1]).any()
    assert len(np.unique(b.core)) > 1 and len(np.unique(b.truss)) > 1 and b.triangles.any()   # a base worth tiling

    core, layer, rounds = cref.peel(t.n, t.edges)
    assert core.dtype == t.core.dtype and np.array_equal(core, t.core)
    assert layer.dtype == t.layer.dtype and np.array_equal(layer, t.layer)
    assert rounds == t.rounds == b.rounds

    canonical, truss, truss_rounds = cref.truss(t.n, t.edges)
    assert np.array_equal(canonical, t.canonical) and np.array_equal(canonical, gsr.canonical_edges(t.n, t.edges))
    assert truss.dtype == t.truss.dtype and np.array_equal(truss, t.truss)
    assert truss_rounds == t.truss_rounds == b.truss_rounds

    triangles = gsr.triangles(t.n, t.edges)
    assert triangles.dtype == t.triangles.dtype and np.array_equal(triangles, t.triangles)
    assert int(triangles.sum()) == 3 * int(b.triangles.sum())

    labels = gsr.component_labels(t.n, t.edges)
    assert labels.dtype == t.labels.dtype and np.array_equal(labels, t.labels)
    assert len(np.unique(labels)) == 3 * len(np.unique(b.labels))


def test_copies_and_seed_are_parameters():
    a, b, c = tiled_graphs.tiled("relaxed_caveman", 2, seed=1), tiled_graphs.tiled("relaxed_caveman", 2, seed=2), \
        tiled_graphs.tiled("relaxed_caveman", 5, seed=1)
    assert a.n == b.n == 720 and c.n == 1800 and len(c.edges) == 5 * 1980
    assert not np.array_equal(a.perm, b.perm) and not np.array_equal(a.core, b.core)
    assert np.array_equal(np.sort(a.core), np.sort(b.core)) and np.array_equal(np.sort(a.truss), np.sort(b.truss))
    again = tiled_graphs.tiled("relaxed_caveman", 2, seed=1)
    assert np.array_equal(a.edges, again.edges) and np.array_equal(a.labels, again.labels)
