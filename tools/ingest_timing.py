#!/usr/bin/env python3
"""Times edge-list ingestion on one synthetic SNAP text (4 M rows by default): load_snap_edge_list's Python loop, the
library's host path, and the device path both with the upload and with the text already on the device; then the host and
the device path on prefixes of the text, to find the size at which the device path overtakes the host path (the value for
datasets.DEVICE_MIN_BYTES).  Prints a markdown table with bytes/s.  Every timing is the best of --repeats runs after one
warm-up run; a timed run ends with the result arrays on the host.

    python tools/ingest_timing.py [--rows 4000000] [--repeats 3] [--skip-python-loop]
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import graphem_rapids_amd as gra  # noqa: E402  pylint: disable=wrong-import-position
from graphem_rapids_amd import _native  # noqa: E402  pylint: disable=wrong-import-position


def synthetic_text(rows, seed=0):
    """SNAP text of `rows` data rows on about rows / 20 labels below 10^8: a header, tab-separated pairs."""
    rng = np.random.default_rng(seed)
    labels = rng.choice(10 ** 8, size=max(2, rows // 20), replace=False)
    pairs = labels[rng.integers(0, len(labels), size=(rows, 2))]
    head = b"# Directed graph: synthetic\n# FromNodeId\tToNodeId\n"
    body = "\n".join("\t".join(map(str, row)) for row in pairs.tolist()).encode() + b"\n"
    return head + body


def best(fn, repeats):
    fn()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return min(times)


def parse_once(handle, data, dev_ptr=None):
    if dev_ptr is None:
        handle.parse(data, "snap", False, "edges")
    else:
        handle.parse_uploaded(data, dev_ptr, "snap", False, "edges")
    return handle.vertices(), handle.edges(True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-python-loop", action="store_true")
    args = ap.parse_args()
    data = np.frombuffer(synthetic_text(args.rows), dtype=np.uint8)
    have_device = _native.device_count() > 0
    host = _native.EdgeListParser(-1)
    dev = _native.EdgeListParser(0) if have_device else None
    rows = []
    if not args.skip_python_loop:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "synthetic.txt")
            data.tofile(path)
            t0 = time.perf_counter()
            want = gra.load_snap_edge_list(path)
            rows.append(("load_snap_edge_list (Python loop), once", time.perf_counter() - t0))
        got = parse_once(host, data)
        assert np.array_equal(got[1], want[1]) and len(got[0]) == len(want[0])
    rows.append(("host path", best(lambda: parse_once(host, data), args.repeats)))
    if have_device:
        import torch
        want = parse_once(host, data)
        got = parse_once(dev, data)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        rows.append(("device path, with upload", best(lambda: parse_once(dev, data), args.repeats)))
        buf = torch.from_numpy(data.copy()).to("cuda:0")
        torch.cuda.synchronize()
        rows.append(("device path, text already on the device", best(lambda: parse_once(dev, data, buf.data_ptr()), args.repeats)))
        t = best(lambda: (dev.parse(data, "snap", True, "edges")), args.repeats)
        rows.append(("device path, with upload, directed, parse only (no copy back)", t))
    print(f"\n{args.rows} rows, {data.size} bytes, best of {args.repeats}\n")
    print("| path | seconds | MB/s |")
    print("|---|---|---|")
    for name, t in rows:
        print(f"| {name} | {t:.4f} | {data.size / t / 1e6:.1f} |")
    if have_device:
        print("\n| bytes | host path s | device path s (with upload) |")
        print("|---|---|---|")
        size = 1 << 12
        while size < data.size:
            end = size + int(np.flatnonzero(data[size:size + 64] == 10)[0]) + 1     # after the next LF
            part = data[:end]
            th = best(lambda: parse_once(host, part), args.repeats)                 # pylint: disable=cell-var-from-loop
            td = best(lambda: parse_once(dev, part), args.repeats)                  # pylint: disable=cell-var-from-loop
            print(f"| {end} | {th:.6f} | {td:.6f} |")
            size *= 4
    host.close()
    if dev:
        dev.close()


if __name__ == "__main__":
    main()
