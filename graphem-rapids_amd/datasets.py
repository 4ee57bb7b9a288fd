"""Real-world edge-list datasets: the reference's datasets.py without its download.

The reference fetches a file and then parses it in a Python loop (datasets.py:306-357, 485-572, 635-683).  Here the file
has to be on disk already -- nothing in this module can reach a network -- and the text of a SNAP `.txt`, a Network
Repository `.edges` or a `.mtx` file is parsed by the library (include/graphem_hip.h "edge-list ingestion"): HIP kernels
when a device is present and the file is large enough, else the library's host path, the same arrays bit for bit.  The
catalogue, the name resolution, the error texts and the return values are the reference's.

Layout on disk, as the reference leaves it: <data directory>/<catalogue key>/<file>, e.g.
data/snap-ca-GrQc/ca-GrQc.txt (or ca-GrQc.txt.gz), data/netrepo-ia-reality/**/ia-reality.mtx,
data/semanticscholar-s2-CS/s2-CS-nodes.csv.  The data directory is $GRAPHEM_DATA_DIR, else `data` beside the package; it
is never created here.
"""
import gzip
import os
from pathlib import Path

import numpy as np

# Below this many bytes read_edge_list(device_id=None) takes the library's host path even with a device present.
# From tools/ingest_timing.py on an MI355X (NOTES.md "Edge-list ingestion", best of 3 on handles that are open already):
#     bytes     host path    device path, with upload
#     16 389    0.090 ms     0.395 ms
#     65 545    0.557 ms     0.439 ms
#    262 160    2.714 ms     0.510 ms
# The device path costs about 0.4 ms whatever the size (some thirty launches, about ten synchronisations); the host path
# reaches that near 50 KB.  64 KiB is the first measured size at which the device wins; opening a handle (a stream, the
# first allocations) is not in these figures and moves the true crossover up a little, not down.
DEVICE_MIN_BYTES = 1 << 16

_SNAP_BASE = "https://snap.stanford.edu/data/"
_NETREPO_BASE = "https://nrvis.com/download/data/"
# key, file at the source, description, directed, nodes, edges
_SNAP = (
    ("facebook_combined", "facebook_combined.txt.gz", "Facebook social network", False, 4039, 88234),
    ("ego-twitter", "twitter_combined.txt.gz", "Twitter ego network", True, 81306, 1768149),
    ("wiki-vote", "wiki-Vote.txt.gz", "Wikipedia who-votes-on-whom network", True, 7115, 103689),
    ("ca-GrQc", "ca-GrQc.txt.gz", "Collaboration network of Arxiv General Relativity", False, 5242, 14496),
    ("ca-HepTh", "ca-HepTh.txt.gz", "Collaboration network of Arxiv High Energy Physics Theory", False, 9877, 25998),
    ("oregon1_010331", "oregon1_010331.txt.gz", "AS peering network from Oregon route views", False, 10670, 22002),
    ("p2p-Gnutella04", "p2p-Gnutella04.txt.gz", "Gnutella peer-to-peer network from August 4, 2002", True, 10876, 39994),
    ("email-Enron", "email-Enron.txt.gz", "Email communication network from Enron", True, 36692, 183831),
)
# key, folder at the source, description, directed, suffix of the data file
_NETREPO = (
    ("soc-hamsterster", "soc", "Hamsterster social network", False, ".mtx"),
    ("socfb-MIT", "socfb", "Facebook network from MIT", False, ".mtx"),
    ("ca-cit-HepPh", "ca", "Citation network of Arxiv High Energy Physics", True, ".mtx"),
    ("web-google-dir", "web", "Google web graph", True, ".edges"),
    ("ia-reality", "ia", "Reality Mining social network", False, ".mtx"),
)
_S2 = (
    ("s2-CS", "https://github.com/mattbierbaum/citation-networks/raw/master/s2-CS.tar.gz",
     "Computer Science citation network from Semantic Scholar"),
)

_device_count = None


def get_data_directory():
    """Where the dataset files are looked for: $GRAPHEM_DATA_DIR, else `data` beside the package.  Not created."""
    env = os.environ.get("GRAPHEM_DATA_DIR")
    return Path(env) if env else Path(__file__).resolve().parent.parent / "data"


def _format_of(path, fmt):
    if fmt != "auto":
        return fmt
    name = str(path)
    if name.endswith(".gz"):
        name = name[:-3]
    return "mtx" if name.endswith(".mtx") else "edges" if name.endswith(".edges") else "snap"


def _read_bytes(path):
    path = Path(path)
    if path.suffix == ".gz":
        with gzip.open(path, "rb") as fh:
            return fh.read()
    return path.read_bytes()


def parse_edge_list(data, format="snap", directed=False, relabel=True, vertices_from="edges", device_id=None,
                    memory_budget=None):   # pylint: disable=redefined-builtin
    """read_edge_list for the bytes of a file that is in memory already."""
    global _device_count
    from . import _native
    if device_id is None:
        if _device_count is None:
            _device_count = int(_native.load().gh_device_count())
        device_id = 0 if _device_count > 0 and len(data) >= DEVICE_MIN_BYTES else -1
    parser = _native.EdgeListParser(device_id)
    try:
        if memory_budget is not None:
            parser.set_memory_budget(memory_budget)
        parser.parse(data, format, directed, vertices_from)
        vertices, edges = parser.vertices(), parser.edges(relabel)
    finally:
        parser.close()
    if relabel:
        vertices = np.arange(len(vertices), dtype=np.int64)
    return vertices, edges


def read_edge_list(path, format="auto", directed=False, relabel=True, vertices_from="edges", device_id=None,
                   memory_budget=None):   # pylint: disable=redefined-builtin
    """A text edge list -> (vertices, edges), both int64, under the rule of include/graphem_hip.h.

    format: 'snap' / 'edges' ('#' comment lines), 'mtx' (the '%' header and the size line are skipped, labels are
    1-based), or 'auto' by suffix after a trailing .gz: .mtx, .edges, anything else snap.  A .gz file is inflated on the
    host first.  directed=False gives the sorted unique pairs u < v; directed=True keeps the rows as they come.
    vertices_from: 'edges' -- the labels of the returned edges (SNAPDataset.load) -- or 'rows' -- of every data row
    (the Network Repository loaders).  relabel=True compacts labels to 0..n-1 in sorted-label order, as
    load_snap_edge_list does; relabel=False returns what the reference's loader returns.  device_id: None picks the
    device when one is present and the file has at least DEVICE_MIN_BYTES bytes, else the library's host path; -1 is the
    host path; >= 0 that device.  A malformed line raises ValueError naming its 1-based line number."""
    return parse_edge_list(_read_bytes(path), _format_of(path, format), directed, relabel, vertices_from, device_id,
                           memory_budget)


class DatasetLoader:
    """What the three sources share.  A loader never creates a directory and never fetches anything."""
    SOURCE = ""
    AVAILABLE_DATASETS = {}

    def __init__(self, dataset_name, prefix, data_dir=None):
        if dataset_name not in self.AVAILABLE_DATASETS:
            raise ValueError(f"Unknown {self.SOURCE} dataset: {dataset_name}. "
                             f"Available datasets: {', '.join(self.AVAILABLE_DATASETS.keys())}")
        self.dataset_name = dataset_name
        self.dataset_info = self.AVAILABLE_DATASETS[dataset_name]
        self.name = f"{prefix}-{dataset_name}"
        self.data_dir = Path(data_dir if data_dir is not None else get_data_directory()) / self.name
        self.url = self.dataset_info["url"]

    def expected_path(self):
        raise NotImplementedError

    def _missing(self, what=None):
        return FileNotFoundError(f"{what or self.expected_path()} is missing and this package downloads nothing: "
                                 f"fetch {self.url} by hand and unpack it into {self.data_dir}")

    def download(self):
        raise RuntimeError(f"this package downloads nothing: fetch {self.url} by hand; the file is expected at "
                           f"{self.expected_path()}")

    def is_downloaded(self):
        return self.expected_path().exists()

    def load(self, relabel=False):
        raise NotImplementedError

    def load_as_networkx(self):
        """networkx.Graph on 0..n-1 in sorted-label order (what convert_node_labels_to_integers leaves)."""
        import networkx as nx
        vertices, edges = self.load(relabel=True)
        G = nx.empty_graph(len(vertices))
        G.add_edges_from(edges.tolist())
        return G

    def info(self):
        if not self.is_downloaded():
            print(f"Dataset '{self.name}' is not downloaded yet.")
            return
        vertices, edges = self.load()
        n, m = len(vertices), len(edges)
        print(f"Dataset: {self.name}")
        print(f"Number of vertices: {n}")
        print(f"Number of edges: {m}")
        print(f"Density: {2 * m / (n * (n - 1)):.6f}")
        print(f"Average degree: {2 * m / n:.2f}")


class SNAPDataset(DatasetLoader):
    """Stanford Network Analysis Project, https://snap.stanford.edu/data/ (reference datasets.py:197-357)."""
    SOURCE = "SNAP"
    AVAILABLE_DATASETS = {key: {"url": _SNAP_BASE + file, "description": text, "directed": directed, "nodes": nodes,
                                "edges": edges} for key, file, text, directed, nodes, edges in _SNAP}

    def __init__(self, dataset_name, data_dir=None):
        super().__init__(dataset_name, "snap", data_dir)
        self.is_directed = self.dataset_info["directed"]

    def expected_path(self):
        return self.data_dir / self.url.split("/")[-1].replace(".gz", "")

    def _path(self):
        plain = self.expected_path()
        if plain.exists():
            return plain
        packed = plain.with_name(plain.name + ".gz")
        if packed.exists():
            return packed
        raise self._missing()

    def is_downloaded(self):
        return self.expected_path().exists() or self.expected_path().with_name(self.expected_path().name + ".gz").exists()

    def load(self, relabel=False, device_id=None):
        return read_edge_list(self._path(), "snap", self.is_directed, relabel, "edges", device_id)


class NetworkRepositoryDataset(DatasetLoader):
    """Network Repository, https://networkrepository.com/ (reference datasets.py:360-572)."""
    SOURCE = "Network Repository"
    AVAILABLE_DATASETS = {key: {"url": f"{_NETREPO_BASE}{folder}/{key}.zip", "description": text, "directed": directed,
                                "file_pattern": key + suffix} for key, folder, text, directed, suffix in _NETREPO}

    def __init__(self, dataset_name, data_dir=None):
        super().__init__(dataset_name, "netrepo", data_dir)
        self.is_directed = self.dataset_info["directed"]
        self.file_pattern = self.dataset_info["file_pattern"]

    def expected_path(self):
        return self.data_dir / self.file_pattern

    def _find_data_file(self):
        matches = list(self.data_dir.glob(f"**/{self.file_pattern}"))
        if not matches:
            raise self._missing(f"a file matching {self.file_pattern} in {self.data_dir}")
        if len(matches) > 1:
            raise RuntimeError(f"Multiple files matched {self.file_pattern} in {self.data_dir}: {matches}")
        return matches[0]

    def load(self, relabel=False, device_id=None):
        path = self._find_data_file()
        if path.suffix not in (".mtx", ".edges"):
            raise ValueError(f"Unsupported file format: {path.suffix}")
        return read_edge_list(path, path.suffix[1:], self.is_directed, relabel, "rows", device_id)


class SemanticScholarDataset(DatasetLoader):
    """Semantic Scholar citation networks (reference datasets.py:575-683): a nodes CSV with an `id` column and a
    citations CSV with `source` and `target`.  The ids are strings, so this source is host only (pandas)."""
    SOURCE = "Semantic Scholar"
    AVAILABLE_DATASETS = {key: {"url": url, "description": text, "nodes_file": key + "-nodes.csv",
                                "edges_file": key + "-citations.csv"} for key, url, text in _S2}

    def __init__(self, dataset_name="s2-CS", data_dir=None):
        super().__init__(dataset_name, "semanticscholar", data_dir)
        self.nodes_file = self.dataset_info["nodes_file"]
        self.edges_file = self.dataset_info["edges_file"]

    def expected_path(self):
        return self.data_dir / self.nodes_file

    def is_downloaded(self):
        return (self.data_dir / self.nodes_file).exists() and (self.data_dir / self.edges_file).exists()

    def load(self, relabel=False):
        import pandas as pd
        for name in (self.nodes_file, self.edges_file):
            if not (self.data_dir / name).exists():
                raise self._missing(self.data_dir / name)
        ids = pd.read_csv(self.data_dir / self.nodes_file)["id"]
        cites = pd.read_csv(self.data_dir / self.edges_file)
        # id -> its position in the nodes file; of a repeated id the last position, as a dict built in order keeps
        index = pd.Series(np.arange(len(ids), dtype=np.int64), index=ids.to_numpy())
        index = index[~index.index.duplicated(keep="last")]
        src = index.reindex(cites["source"].to_numpy()).to_numpy(dtype=np.float64)
        dst = index.reindex(cites["target"].to_numpy()).to_numpy(dtype=np.float64)
        known = ~(np.isnan(src) | np.isnan(dst))
        rows = np.column_stack([src[known], dst[known]]).astype(np.int64).reshape(-1, 2)
        vertices = np.unique(rows.ravel())
        lo, hi = np.minimum(rows[:, 0], rows[:, 1]), np.maximum(rows[:, 0], rows[:, 1])
        keep = lo < hi
        edges = np.unique(np.column_stack([lo[keep], hi[keep]]), axis=0).reshape(-1, 2)
        if relabel:
            edges = np.searchsorted(vertices, edges)
            vertices = np.arange(len(vertices), dtype=np.int64)
        return vertices, edges


_SOURCES = (("snap-", SNAPDataset), ("netrepo-", NetworkRepositoryDataset), ("semanticscholar-", SemanticScholarDataset))


def _loader(dataset_name, data_dir=None):
    """The reference's resolution (datasets.py:739-758): the three prefixes first, then a bare catalogue key; of several
    matches the last one wins, and a prefix with an unknown key raises that source's message."""
    loader = None
    for prefix, cls in _SOURCES:
        if dataset_name.startswith(prefix):
            loader = cls(dataset_name[len(prefix):], data_dir)
    for _, cls in _SOURCES:
        if dataset_name in cls.AVAILABLE_DATASETS:
            loader = cls(dataset_name, data_dir)
    if loader is None:
        raise ValueError(f"Unknown dataset: {dataset_name}")
    return loader


def list_available_datasets():
    """{catalogue key: facts}, with the reference's keys and values (datasets.py:686-723)."""
    out = {}
    for name, info in SNAPDataset.AVAILABLE_DATASETS.items():
        out[f"snap-{name}"] = {"source": "SNAP", "name": name, "description": info["description"],
                               "nodes": info.get("nodes", "Unknown"), "edges": info.get("edges", "Unknown"),
                               "directed": info["directed"]}
    for name, info in NetworkRepositoryDataset.AVAILABLE_DATASETS.items():
        out[f"netrepo-{name}"] = {"source": "Network Repository", "name": name, "description": info["description"],
                                  "directed": info["directed"]}
    for name, info in SemanticScholarDataset.AVAILABLE_DATASETS.items():
        out[f"semanticscholar-{name}"] = {"source": "Semantic Scholar", "name": name, "description": info["description"]}
    return out


def load_dataset(dataset_name, data_dir=None, relabel=False):
    """(vertices, edges) of a catalogue dataset whose file is on disk, as the reference's load_dataset returns them;
    relabel=True compacts the labels to 0..n-1.  A missing file raises FileNotFoundError with the path and the URL."""
    return _loader(dataset_name, data_dir).load(relabel=relabel)


def load_dataset_as_networkx(dataset_name, data_dir=None):
    """networkx.Graph on 0..n-1 (datasets.py:761-782)."""
    return _loader(dataset_name, data_dir).load_as_networkx()


def load_dataset_adjacency(dataset_name, data_dir=None):
    """The symmetric CSR adjacency of ones that create_graphem takes: vertices 0..n-1 in sorted-label order; directions,
    repeats and self-loops of the file are merged away."""
    from .generators import edges_to_adjacency
    vertices, edges = _loader(dataset_name, data_dir).load(relabel=True)
    keep = edges[:, 0] != edges[:, 1]
    return edges_to_adjacency(len(vertices), edges[keep])
