"""A scipy / numpy restatement of what gh_cent_paths and gh_cent_pagerank compute (include/graphem_hip.h "centrality"),
level-synchronous like the kernels, for checks at sizes networkx cannot reach.  tests/test_centrality_cpu.py checks it
against networkx on small graphs.

For a batch of sources at once (rows = sources, columns = vertices):
    forward   sigma_L = (frontier sigma of level L - 1) @ A on the unvisited entries; npred likewise with 0/1 frontiers
    backward  delta(x) = sigma(x) * (A @ ((1 + delta(w)) / sigma(w) on level L + 1))(x)    for x on level L
              lam(x)   = (A @ ((1 + lam(w)) / npred(w) on level L + 1))(x)
Returns raw (unnormalised) sums over the sources, the source itself excluded, and per-source reached counts and
distance sums."""
import numpy as np
import scipy.sparse as sp


def adjacency(n, edges):
    """Symmetric 0/1 CSR, self-loops dropped, duplicates merged."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    e = e[e[:, 0] != e[:, 1]]
    a = sp.coo_matrix((np.ones(2 * len(e)), (np.r_[e[:, 0], e[:, 1]], np.r_[e[:, 1], e[:, 0]])), shape=(n, n)).tocsr()
    a.data[:] = 1.0
    a.sum_duplicates()
    a.data[:] = 1.0
    return a


def paths(n, edges, sources, batch=256):
    """(betweenness (n,), load (n,), reached (S,), dist_sum (S,)): raw sums over `sources`."""
    A = adjacency(n, edges)
    AT = A.T.tocsr()
    sources = np.asarray(sources, dtype=np.int64)
    bc = np.zeros(n)
    ld = np.zeros(n)
    reached = np.zeros(len(sources), dtype=np.int64)
    dsum = np.zeros(len(sources), dtype=np.int64)
    for b0 in range(0, len(sources), batch):
        src = sources[b0:b0 + batch]
        S = len(src)
        rows = np.arange(S)
        dist = np.full((S, n), -1, dtype=np.int64)
        sigma = np.zeros((S, n))
        npred = np.zeros((S, n))
        dist[rows, src] = 0
        sigma[rows, src] = 1.0
        front = np.zeros((S, n), dtype=bool)
        front[rows, src] = True
        L = 0
        while front.any():
            L += 1
            s_in = np.where(front, sigma, 0.0)
            new_sigma = np.asarray((AT @ s_in.T).T)            # sum of sigma over the frontier neighbours
            new_cnt = np.asarray((AT @ front.T.astype(np.float64)).T)
            nxt = (dist < 0) & (new_cnt > 0)
            dist[nxt] = L
            sigma[nxt] = new_sigma[nxt]
            npred[nxt] = new_cnt[nxt]
            front = nxt
        maxd = L - 1
        delta = np.zeros((S, n))
        lam = np.zeros((S, n))
        for L in range(maxd, 0, -1):
            on_next = dist == L + 1
            coeff = np.where(on_next, (1.0 + delta) / np.where(on_next, sigma, 1.0), 0.0)
            q = np.where(on_next, (1.0 + lam) / np.where(on_next, npred, 1.0), 0.0)
            here = dist == L
            cd = np.asarray((A @ coeff.T).T)
            cq = np.asarray((A @ q.T).T)
            delta[here] = sigma[here] * cd[here]
            lam[here] = cq[here]
        inside = dist >= 1
        bc += np.where(inside, delta, 0.0).sum(axis=0)
        ld += np.where(inside, lam, 0.0).sum(axis=0)
        reached[b0:b0 + S] = (dist >= 0).sum(axis=1)
        dsum[b0:b0 + S] = np.where(dist >= 0, dist, 0).sum(axis=1)
    return bc, ld, reached, dsum


def pagerank(n, edges, alpha=0.85, max_iter=100, tol=1e-6, changes=None):
    """networkx _pagerank_scipy restated: (x, iterations); iterations = -1 when max_iter iterations did not converge.
    changes (a list) receives every iteration's L1 change, the number that is held against n tol."""
    A = adjacency(n, edges)
    S = np.asarray(A.sum(axis=1)).ravel()
    inv = np.zeros(n)
    inv[S != 0] = 1.0 / S[S != 0]
    M = sp.diags(inv) @ A
    x = np.repeat(1.0 / n, n)
    p = np.repeat(1.0 / n, n)
    dangling = np.where(S == 0)[0]
    for it in range(1, max_iter + 1):
        xlast = x
        x = alpha * (x @ M + sum(x[dangling]) * p) + (1 - alpha) * p
        err = np.absolute(x - xlast).sum()
        if changes is not None:
            changes.append(float(err))
        if err < n * tol:
            return x, it
    return x, -1
