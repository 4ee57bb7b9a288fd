"""Small deterministic texts in the three Network Repository / Semantic Scholar shapes (numpy PCG64), a few thousand
rows each: repeats, both directions of some pairs, a vertex that occurs only in a self-loop, a weight column, labels that
are not contiguous.  tests/golden/datasets_ref.npz holds the sha1 of each text and what the REFERENCE's own loaders
returned for it (tests/golden/make_golden_datasets.py)."""
import hashlib

import numpy as np

N_ROWS = 3000


def _rows(seed, n_labels, low):
    rng = np.random.default_rng(seed)
    labels = np.sort(rng.choice(20 * n_labels, size=n_labels, replace=False)).astype(np.int64) + low
    a, b = rng.integers(0, n_labels - 1, size=N_ROWS), rng.integers(0, n_labels - 1, size=N_ROWS)
    rows = [(int(labels[x]), int(labels[y])) for x, y in zip(a, b)]
    for i in rng.choice(N_ROWS, size=150, replace=False):     # reversed repeats and plain repeats
        rows.append((rows[i][1], rows[i][0]))
    for i in rng.choice(N_ROWS, size=100, replace=False):
        rows.append(rows[i])
    for i in rng.choice(n_labels - 1, size=25, replace=False):
        rows.append((int(labels[i]), int(labels[i])))
    order = rng.permutation(len(rows))
    rows = [rows[i] for i in order]
    lonely = int(labels[n_labels - 1])                         # occurs in this self-loop only
    rows.insert(len(rows) // 2, (lonely, lonely))
    return rows, rng


def mtx_text(seed=31):
    """Matrix Market coordinate text: a banner, '%' comments, the size line, then 1-based rows with a weight column."""
    rows, rng = _rows(seed, 400, 1)
    out = ["%%MatrixMarket matrix coordinate real general", "% synthetic", "%", "8000 8000 %d" % len(rows)]
    for i, (a, b) in enumerate(rows):
        out.append("%d %d %s" % (a, b, ("0.5", "1e-3", "7")[i % 3]))
    return "\n".join(out) + "\n"


def edges_text(seed=47):
    """Network Repository .edges text: '#' comments at the top and in the middle, separators of several kinds, a weight
    column on some rows, a blank line, no terminator after the last row."""
    rows, rng = _rows(seed, 500, 0)
    seps = [" ", "\t", "  ", " \t"]
    out = ["# synthetic .edges file", "# u v w"]
    pick = rng.integers(0, len(seps), size=len(rows))
    for i, (a, b) in enumerate(rows):
        if i % 1000 == 999:
            out.append("# a comment in the middle")
        if i == 77:
            out.append("")
        out.append("%d%s%d%s" % (a, seps[pick[i]], b, " 0.25" if i % 5 == 0 else ""))
    return "\n".join(out)


def s2_csvs(seed=59):
    """(nodes csv, citations csv) of the Semantic Scholar pair: string ids, some citations of papers that are no node."""
    rng = np.random.default_rng(seed)
    n = 600
    ids = ["p%05x" % v for v in rng.choice(1 << 20, size=n, replace=False)]
    nodes = "id,title\n" + "".join("%s,paper %d\n" % (s, i) for i, s in enumerate(ids))
    src, dst = rng.integers(0, n, size=N_ROWS), rng.integers(0, n, size=N_ROWS)
    lines = ["source,target"]
    for i, (a, b) in enumerate(zip(src, dst)):
        s, t = ids[a], ids[b]
        if i % 97 == 0:
            t = "unknown%d" % i
        if i % 101 == 0:
            s = "missing%d" % i
        lines.append("%s,%s" % (s, t))
        if i % 13 == 0:
            lines.append("%s,%s" % (t, s))
        if i % 211 == 0:
            lines.append("%s,%s" % (s, s))
    return nodes, "\n".join(lines) + "\n"


def text_sha1(text):
    return hashlib.sha1(text.encode("utf-8")).hexdigest()
