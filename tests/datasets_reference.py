"""The edge-list parsing rule of include/graphem_hip.h restated in plain Python, the way the reference reads a file: a
text-mode open (universal newlines), a loop over lines, startswith for comments, strip().split() for fields, int() for
labels, numpy's unique for the results.  Where the rule deviates from Python on purpose -- an underscore in a number, a
non-ASCII digit -- this raises ValueError as the rule does.  (The rule's other deviation, U+0085 / U+00A0 as blanks, is
not restated: no test text holds them.)"""
import io

import numpy as np

INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1


def _label(field, lineno, dec):
    if not field.isascii() or "_" in field:
        raise ValueError(f"line {lineno}: {field!r}")
    try:
        value = int(field)
    except ValueError:
        raise ValueError(f"line {lineno}: {field!r}") from None
    if not INT64_MIN <= value <= INT64_MAX or not INT64_MIN <= value - dec:
        raise ValueError(f"line {lineno}: {field!r}")
    return value - dec


def rows_of(data, fmt="snap"):
    """[(a, b)] of the data rows of the bytes of a file, in file order."""
    fh = io.TextIOWrapper(io.BytesIO(bytes(data)), encoding="utf-8", newline=None)   # what open(path, 'r') gives
    lines = iter(fh)
    lineno, rows = 0, []
    if fmt == "mtx":
        for line in lines:
            lineno += 1
            if not line.startswith("%"):
                break                                   # the size line, whatever it holds
    for line in lines:
        lineno += 1
        if fmt != "mtx" and line.startswith("#"):
            continue
        parts = line.strip().split()
        if len(parts) >= 2:
            rows.append((_label(parts[0], lineno, fmt == "mtx"), _label(parts[1], lineno, fmt == "mtx")))
    return rows


def parse(data, fmt="snap", directed=False, relabel=False, vertices_from="edges"):
    """(vertices, edges) int64 under the rule."""
    rows = np.array(rows_of(data, fmt), dtype=np.int64).reshape(-1, 2)
    edges = rows
    if not directed:
        lo, hi = np.minimum(rows[:, 0], rows[:, 1]), np.maximum(rows[:, 0], rows[:, 1])
        keep = lo < hi
        edges = np.unique(np.column_stack([lo[keep], hi[keep]]), axis=0).reshape(-1, 2)
    vertices = np.unique((rows if vertices_from == "rows" else edges).ravel())
    if relabel:
        edges = np.searchsorted(vertices, edges)
        vertices = np.arange(len(vertices), dtype=np.int64)
    return vertices, edges
