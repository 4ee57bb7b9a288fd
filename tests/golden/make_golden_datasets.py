#!/usr/bin/env python3
"""tests/golden/datasets_ref.npz: what the REFERENCE's own loaders return for the texts of tests/datasets_synth.py --
NetworkRepositoryDataset._load_mtx_file and ._load_edges_file, each directed and undirected, and
SemanticScholarDataset.load -- with the sha1 of every text.  The outputs are data.  Run once on a CPU:

    python tests/golden/make_golden_datasets.py <checkout of the reference>

The loader objects are made with object.__new__: the constructors only build download paths and directories.  loguru is
stood in for by the logging module; nothing is fetched."""
import importlib.util
import logging
import os
import pathlib
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import datasets_synth  # noqa: E402  pylint: disable=wrong-import-position


def _reference_datasets(ref):
    stub = types.ModuleType("loguru")
    stub.logger = logging.getLogger("loguru-stub")
    sys.modules["loguru"] = stub
    for name in ("requests", "tqdm"):                 # named by the module's imports, never called here
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
            sys.modules[name].tqdm = None
    spec = importlib.util.spec_from_file_location("reference_datasets", os.path.join(ref, "graphem_rapids", "datasets.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(ref):
    ds = _reference_datasets(ref)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        for kind, text, load in (("mtx", datasets_synth.mtx_text(), "_load_mtx_file"),
                                 ("edges", datasets_synth.edges_text(), "_load_edges_file")):
            path = tmp / ("synth." + kind)
            path.write_text(text, encoding="utf-8")
            out[kind + "_text_sha1"] = np.array(datasets_synth.text_sha1(text))
            for directed in (False, True):
                ld = object.__new__(ds.NetworkRepositoryDataset)
                ld.is_directed = directed
                vertices, edges = getattr(ld, load)(path)
                tag = kind + ("_directed" if directed else "_undirected")
                out[tag + "_vertices"] = np.asarray(vertices, dtype=np.int64)
                out[tag + "_edges"] = np.asarray(edges, dtype=np.int64)
        nodes, cites = datasets_synth.s2_csvs()
        ld = object.__new__(ds.SemanticScholarDataset)
        ld.data_dir = tmp
        ld.nodes_file, ld.edges_file = "s2-CS-nodes.csv", "s2-CS-citations.csv"
        (tmp / ld.nodes_file).write_text(nodes, encoding="utf-8")
        (tmp / ld.edges_file).write_text(cites, encoding="utf-8")
        vertices, edges = ld.load()
        out["s2_text_sha1"] = np.array(datasets_synth.text_sha1(nodes + cites))
        out["s2_vertices"] = np.asarray(vertices, dtype=np.int64)
        out["s2_edges"] = np.asarray(edges, dtype=np.int64)
    np.savez_compressed(os.path.join(HERE, "datasets_ref.npz"), **out)
    print({k: (v.shape if v.shape else str(v)[:12]) for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1])
