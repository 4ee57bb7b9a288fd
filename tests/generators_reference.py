"""Plain restatement of the three counter-based generator rules, written from the text of include/graphem_hip.h
("graph generators"): Python integers, simple loops, brute force where that is simplest.  It is the definition the library
(device kernels and host path alike) is compared with bit for bit; it shares no code with either."""
import numpy as np

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
SEGMENT = 16384      # GH_GEN_SBM_SEGMENT
TABLE = 1024         # GH_GEN_SBM_TABLE


def mix(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
    return z ^ (z >> 31)


def word(seed, i, j):
    return mix(mix((seed + (i + 1) * G) & M64) ^ j)


def _sorted_edges(pairs):
    pairs = sorted(set((min(u, v), max(u, v)) for u, v in pairs))
    return np.array(pairs, dtype=np.int64).reshape(-1, 2)


# ---- block model ----------------------------------------------------------------------------------------------------
def gap_table(p):
    q = 1.0 - p
    pw, out = 1.0, []
    for _ in range(TABLE):
        pw = pw * q
        out.append(int(np.floor((1.0 - pw) * 2.0 ** 52)))
    return out


def _pair(a, b, off, sizes, i):
    if a < b:
        return off[a] + i // sizes[b], off[b] + i % sizes[b]
    s = sizes[a]
    h = (s - 1) // 2
    if i < s * h:
        r, c = i // h, i % h
        return off[a] + r, off[a] + (r + 1 + c) % s
    r = i - s * h
    return off[a] + r, off[a] + r + s // 2


def sbm_edges(sizes, P, seed):
    sizes = [int(s) for s in sizes]
    B = len(sizes)
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    edges = []
    g = 0                                   # running segment number
    for a in range(B):
        for b in range(a, B):
            N = sizes[a] * (sizes[a] - 1) // 2 if a == b else sizes[a] * sizes[b]
            cdf = np.array(gap_table(float(P[a][b])), dtype=np.uint64)      # non-decreasing
            for lo in range(0, N, SEGMENT):
                hi = min(lo + SEGMENT, N)
                pos, j = lo, 0
                while pos < hi:
                    r = word(seed, g, j) >> 12
                    j += 1
                    k = int(np.searchsorted(cdf, np.uint64(r), side="right"))      # entries <= r
                    if k == TABLE:
                        pos += TABLE
                        continue
                    pos += k
                    if pos < hi:
                        edges.append(_pair(a, b, off, sizes, pos))
                    pos += 1
                g += 1
    return _sorted_edges(edges)


# ---- random geometric graph -----------------------------------------------------------------------------------------
def geometric_coords(n, dim, seed):
    return np.array([[word(seed, i, d) >> 40 for d in range(dim)] for i in range(n)], dtype=np.int64).reshape(n, dim)


def geometric_r2(radius):
    return int(np.floor(min(radius * radius, 16.0) * 2.0 ** 48))


def geometric_edges(n, radius, dim, seed):
    """(edges, positions): every pair tested."""
    k = geometric_coords(n, dim, seed)
    r2 = geometric_r2(radius)
    edges = []
    for u in range(n):
        d2 = ((k[u + 1:] - k[u]) ** 2).sum(axis=1)      # int64: at most 8 * 2^48
        for v in np.nonzero(d2 <= r2)[0]:
            edges.append((u, u + 1 + int(v)))
    return _sorted_edges(edges), (k.astype(np.float64) / 2.0 ** 24).astype(np.float32)


# ---- preferential attachment ----------------------------------------------------------------------------------------
def ba_edges(n, m, seed):
    slots = []
    for i in range(m):
        slots += [0, i + 1]
    edges = [(0, i + 1) for i in range(m)]
    for v in range(m + 1, n):
        length = 2 * m * (v - m)
        assert length == len(slots)
        targets, a = [], 0
        while len(targets) < m:
            x = slots[(word(seed, v, a) * length) >> 64]
            a += 1
            if x not in targets:
                targets.append(x)
        for x in targets:
            slots += [v, x]
            edges.append((x, v))
    return _sorted_edges(edges)
