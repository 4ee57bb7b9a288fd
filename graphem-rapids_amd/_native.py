"""ctypes binding of libgraphem_hip.so (include/graphem_hip.h).

There is no CPU fallback: if the library is missing or no MI355X is visible the HIP
backend raises.  Nothing here imports the oracle.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgraphem_hip.so")

GH_OK, GH_ERR_INVALID, GH_ERR_RUNTIME, GH_ERR_K_TOO_LARGE, GH_ERR_HIP, GH_ERR_NOMEM = range(6)


class GhParams(ctypes.Structure):
    _fields_ = [("L_min", ctypes.c_float), ("k_attr", ctypes.c_float), ("k_inter", ctypes.c_float),
                ("n_neighbors", ctypes.c_int32), ("sample_size", ctypes.c_int32), ("seed", ctypes.c_uint64),
                ("reorder", ctypes.c_int32), ("knn_method", ctypes.c_int32), ("knn_distance", ctypes.c_int32),
                ("ivf_lists", ctypes.c_int32), ("ivf_probes", ctypes.c_int32)]


REORDER = {"auto": 0, "off": 1, "bfs": 2}  # gh_params.reorder (include/graphem_hip.h GH_REORDER_*)
KNN_METHOD = {"auto": 0, "scan": 1, "grid": 2, "ivf": 3}  # gh_params.knn_method (GH_KNN_*)
KNN_DISTANCE = {"exact": 0, "cdist": 1}  # gh_params.knn_distance (GH_DIST_*)


class GhPartition(ctypes.Structure):
    _fields_ = [("row_lo", ctypes.c_int64), ("row_hi", ctypes.c_int64),
                ("edge_lo", ctypes.c_int64), ("edge_hi", ctypes.c_int64), ("edge_rule", ctypes.c_int32)]


EDGES_RANGE, EDGES_HASHED = 0, 1  # gh_partition.edge_rule (include/graphem_hip.h)


SCAN_FILTERS = {"auto": 0, "mfma": 1, "cells": 2}  # GH_FILTER_* (include/graphem_hip.h)
COARSE_TAU = {"auto": 0, "off": 1, "on": 2}        # GH_COARSE_*
COMPACT_GATHER = {"off": 0, "on": 1, "auto": 2}    # GH_COMPACT_*
COARSE_GROUPS = 64                                 # GH_CT_M (csrc/engine.h)
LINK_KINDS = {"common_neighbors": 0, "jaccard": 1, "adamic_adar": 2, "resource_allocation": 3,
              "preferential_attachment": 4}  # GH_LINK_* (include/graphem_hip.h)
LINK_MAX_K = 128
KNN_MAX_K = 128             # gh_qual_knn_vote's bound on k
LABEL_MAX_CLASSES = 1024    # gh_cent_label_propagation's bound on n_classes


# Every symbol include/graphem_hip.h declares: name -> (restype, argtypes).  load() applies the table, so a symbol cannot be
# bound without a signature (ctypes would pass its 64-bit pointers as int).
vp, i32, i64, u64, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_double
_int, _str, _P = ctypes.c_int, ctypes.c_char_p, ctypes.POINTER
SIGNATURES = {
    "gh_create": (_int, [_P(vp), _int, i64, i32, i64, vp, _P(GhParams), _P(GhPartition)]),
    "gh_destroy": (None, [vp]),
    "gh_last_error": (_str, [vp]),
    "gh_set_positions": (_int, [vp, vp]),
    "gh_get_positions": (_int, [vp, vp]),
    "gh_positions_device": (vp, [vp]),
    "gh_row_stride": (i32, [vp]),
    "gh_step": (_int, [vp, vp]),
    "gh_run": (_int, [vp, i32, vp]),
    "gh_sync": (_int, [vp]),
    "gh_spring_forces": (_int, [vp, vp]),
    "gh_knn_midpoints": (_int, [vp, vp, vp]),
    "gh_intersection_forces": (_int, [vp, vp, vp, vp]),
    "gh_integrate_normalise": (_int, [vp, vp, vp, vp]),
    "gh_step_begin": (_int, [vp, vp]),
    "gh_knn_partial_device": (vp, [vp]),
    "gh_knn_partial_cols": (i32, [vp]),
    "gh_knn_merged_device": (vp, [vp]),
    "gh_rows_packed_device": (vp, [vp]),
    "gh_step_unpack_rows": (_int, [vp]),
    "gh_set_packed_rows": (_int, [vp, i32]),
    "gh_step_merge": (_int, [vp, vp, i32]),
    "gh_stats_partial_device": (vp, [vp]),
    "gh_step_finish": (_int, [vp]),
    "gh_timing_enable": (_int, [vp, i32]),
    "gh_timing_reset": (_int, [vp]),
    "gh_timing_count": (i32, [vp]),
    "gh_timing_get": (_int, [vp, i32, _P(_str), _P(f64), _P(i64)]),
    "gh_device_count": (i32, []),
    "gh_version": (_str, []),
    "gh_debug_live_allocations": (None, [_P(i64), _P(i64)]),
    "gh_knn_last_counts": (_int, [vp, vp, vp, vp]),
    "gh_set_stream": (_int, [vp, vp, i32]),
    "gh_positions_rows_allocated": (i64, [vp]),
    "gh_knn_points": (_int, [_int, vp, i64, vp, i64, i32, i32, vp]),
    "gh_stats_rows": (i32, [vp]),
    "gh_spmv_symnorm": (_int, [vp, i64, vp, vp, vp, vp, vp]),
    "gh_spectral_last_error": (_str, []),
    "gh_gather_layout": (_int, [vp, i32, i32, i64]),
    "gh_gather_buffer_device": (vp, [vp]),
    "gh_gather_slot_bytes": (i64, [vp]),
    "gh_step_finish_gathered": (_int, [vp]),
    "gh_vertex_order": (_int, [vp, vp]),
    "gh_positions_unpadded_device": (vp, [vp]),
    "gh_radial_topk": (_int, [vp, i32, vp]),
    "gh_comm_unique_id": (_int, [vp]),
    "gh_comm_init_rccl": (_int, [vp, i32, i32, vp]),
    "gh_loopback_group_create": (vp, [i32]),
    "gh_loopback_group_destroy": (None, [vp]),
    "gh_comm_init_loopback": (_int, [vp, vp, i32]),
    "gh_comm_destroy": (_int, [vp]),
    "gh_run_partitioned": (_int, [vp, i32, vp]),
    "gh_comm_last_error": (_str, []),
    "gh_debug_stamps": (_int, [vp, vp, i64]),
    "gh_knn_cdist_stats": (_int, [vp, vp, vp]),
    "gh_rank_layout": (_int, [vp, i32, i32, i64]),
    "gh_step_finish_own": (_int, [vp, vp, i32]),
    "gh_comm_available": (i32, []),
    "gh_selftest_arith": (_int, [_int, u64, i64, _P(i64), _P(i64)]),
    "gh_create_f64": (_int, [_P(vp), _int, i64, i32, i64, vp, _P(GhParams), f64, f64, f64]),
    "gh_set_positions_f64": (_int, [vp, vp]),
    "gh_get_positions_f64": (_int, [vp, vp]),
    "gh_positions_device_f64": (vp, [vp]),
    "gh_spring_forces_f64": (_int, [vp, vp]),
    "gh_intersection_forces_f64": (_int, [vp, vp, vp, vp]),
    "gh_trlan_sweep": (_int, [vp, i64, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp]),
    "gh_knn_ivf_config": (_int, [vp, vp, vp]),
    "gh_knn_ivf_list_sizes": (_int, [vp, vp, i32]),
    "gh_torch_randperm_prefix": (_int, [vp, i64, i64, i64, i32, vp]),
    "gh_torch_randperm_isa": (_str, []),
    "gh_run_torch_sampled": (_int, [vp, i32, vp, i64]),
    "gh_set_cdist_replay": (_int, [vp, i32]),
    "gh_set_scan_filter": (_int, [vp, i32]),
    "gh_get_scan_filter": (_int, [vp, _P(i32)]),
    "gh_set_coarse_tau": (_int, [vp, i32]),
    "gh_get_coarse_tau": (_int, [vp, _P(i32)]),
    "gh_debug_coarse_table": (_int, [vp, vp, i64]),
    "gh_set_compact_gather": (_int, [vp, i32]),
    "gh_get_compact_gather": (_int, [vp, _P(i32)]),
    "gh_compact_gather_launches": (_int, [vp, _P(i64)]),
    "gh_compact_slot": (i64, [i64]),
    "gh_compact_slots": (_int, [i64, i64, vp]),
    "gh_compact_bytes": (i64, [i64]),
    "gh_qcell_probe": (_int, [vp, i32, vp, vp, vp, i64, vp, vp]),
    "gh_sampler_stats": (_int, [vp, vp]),
    "gh_overlap_layout": (_int, [vp, i32, i32, i64]),
    "gh_rows_all_device": (vp, [vp]),
    "gh_rows_all_row_floats": (i32, [vp]),
    "gh_stats_all_device": (vp, [vp]),
    "gh_stats_all_block_doubles": (i64, [vp]),
    "gh_step_rows_early": (i32, [vp]),
    "gh_step_pack_rows": (_int, [vp, vp, i32]),
    "gh_step_finish_overlap": (_int, [vp]),
    "gh_ic_create": (_int, [_P(vp), _int, i64, i64, vp, i32]),
    "gh_ic_destroy": (None, [vp]),
    "gh_ic_last_error": (_str, [vp]),
    "gh_ic_arc_count": (i64, [vp]),
    "gh_ic_set_memory_budget": (_int, [vp, i64]),
    "gh_ic_spread": (_int, [vp, f64, i32, i32, u64, i64, vp, vp, vp, i64, vp, vp]),
    "gh_ic_rr_sample": (_int, [vp, vp, f64, i32, u64, i64, vp, vp]),
    "gh_ic_set_arc_probabilities": (_int, [vp, i64, vp, vp]),
    "gh_ic_spread_arcs": (_int, [vp, i32, i32, u64, i64, vp, vp, vp, i64, vp, vp]),
    "gh_ic_rr_sample_arcs": (_int, [vp, vp, i32, u64, i64, vp, vp]),
    "gh_ic_set_lt_weights": (_int, [vp, i64, vp, vp]),
    "gh_ic_spread_lt": (_int, [vp, i32, i32, u64, i64, vp, vp, vp, i64, vp, vp]),
    "gh_ic_rr_sample_lt": (_int, [vp, vp, i32, u64, i64, vp, vp]),
    "gh_rr_create": (_int, [_P(vp), _int, i64]),
    "gh_rr_destroy": (None, [vp]),
    "gh_rr_last_error": (_str, [vp]),
    "gh_rr_set_memory_budget": (_int, [vp, i64]),
    "gh_rr_counts": (_int, [vp, _P(i64), _P(i64)]),
    "gh_rr_download": (_int, [vp, vp, vp, vp]),
    "gh_rr_upload": (_int, [vp, i64, vp, vp, vp]),
    "gh_rr_cover": (_int, [vp, i64, vp, vp]),
    "gh_rr_count_hit": (_int, [vp, vp, i64, _P(i64)]),
    "gh_cent_create": (_int, [_P(vp), _int, i64, i64, vp]),
    "gh_cent_destroy": (None, [vp]),
    "gh_cent_last_error": (_str, [vp]),
    "gh_cent_edge_count": (i64, [vp]),
    "gh_cent_csr_device": (_int, [vp, _P(vp), _P(vp)]),
    "gh_cent_set_memory_budget": (_int, [vp, i64]),
    "gh_cent_paths": (_int, [vp, i64, vp, vp, vp, vp, vp]),
    "gh_cent_pagerank": (_int, [vp, f64, i32, f64, vp, _P(i32)]),
    "gh_spmv_adj_shift": (_int, [vp, i64, vp, vp, f64, vp, vp]),
    "gh_cent_components": (_int, [vp, vp, _P(i64)]),
    "gh_cent_distances": (_int, [vp, i64, vp, vp, vp, vp]),
    "gh_cent_triangles": (_int, [vp, vp]),
    "gh_cent_cores": (_int, [vp, vp, vp, _P(i32)]),
    "gh_cent_truss": (_int, [vp, vp, _P(i32)]),
    "gh_cent_modularity": (_int, [vp, vp, vp]),
    "gh_cent_louvain": (_int, [vp, u64, i32, i32, vp, _P(i32), vp, vp, vp]),
    "gh_link_weight": (i64, [i32, i64]),
    "gh_cent_link_scores": (_int, [vp, i64, vp, vp, vp, vp]),
    "gh_cent_link_candidates": (_int, [vp, i32, i32, i64, vp, vp, vp, vp]),
    "gh_cent_label_propagation": (_int, [vp, i32, vp, i32, vp, _P(i32), _P(i32)]),
    "gh_gen_create": (_int, [_P(vp), _int]),
    "gh_gen_destroy": (None, [vp]),
    "gh_gen_last_error": (_str, [vp]),
    "gh_gen_set_memory_budget": (_int, [vp, i64]),
    "gh_gen_sbm": (_int, [vp, i32, vp, vp, u64, _P(i64)]),
    "gh_gen_geometric": (_int, [vp, i64, f64, i32, u64, _P(i64)]),
    "gh_gen_ba": (_int, [vp, i64, i64, u64, _P(i64), _P(i32)]),
    "gh_gen_edges": (_int, [vp, vp]),
    "gh_gen_positions": (_int, [vp, vp]),
    "gh_corr_create": (_int, [_P(vp), _int, i64, i32, vp]),
    "gh_corr_destroy": (None, [vp]),
    "gh_corr_last_error": (_str, [vp]),
    "gh_corr_set_memory_budget": (_int, [vp, i64]),
    "gh_corr_rho": (f64, [i64, i64, i64]),
    "gh_corr_matrix": (_int, [vp, vp, vp]),
    "gh_corr_bootstrap": (_int, [vp, i32, vp, i32, u64, vp, vp]),
    "gh_qual_create": (_int, [_P(vp), _int, i64, i64, vp]),
    "gh_qual_destroy": (None, [vp]),
    "gh_qual_last_error": (_str, [vp]),
    "gh_qual_set_positions": (_int, [vp, vp, i32, i64, i32]),
    "gh_qual_crossings": (_int, [vp, i64, vp, vp, _P(i64)]),
    "gh_qual_pairs": (_int, [vp, i64, vp, vp]),
    "gh_qual_edge_lengths": (_int, [vp, vp]),
    "gh_qual_neighbor_sizes": (_int, [vp, i64, vp, vp]),
    "gh_qual_neighbor_ranks": (_int, [vp, i64, vp, vp, vp, vp, vp]),
    "gh_qual_hop_profile": (_int, [vp, i64, vp, i64, _P(i64), vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "gh_qual_position_rows": (_int, [vp, i64, vp, vp]),
    "gh_qual_kmeans_assign": (_int, [vp, i32, vp, vp, vp]),
    "gh_qual_kmeans": (_int, [vp, i32, vp, i32, vp, vp, vp, _P(i32), _P(i32)]),
    "gh_qual_kmeans_seed_step": (_int, [vp, i64, i32, vp]),
    "gh_qual_cluster_distance_sums": (_int, [vp, i32, vp, i64, vp, vp]),
    "gh_qual_knn_vote": (_int, [vp, i32, i64, vp, vp, i64, vp, vp, vp, vp, vp]),
    "gh_ingest_create": (_int, [_P(vp), _int]),
    "gh_ingest_destroy": (None, [vp]),
    "gh_ingest_last_error": (_str, [vp]),
    "gh_ingest_set_memory_budget": (_int, [vp, i64]),
    "gh_ingest_parse": (_int, [vp, vp, i64, i32, i32, i32]),
    "gh_ingest_parse_uploaded": (_int, [vp, vp, vp, i64, i32, i32, i32]),
    "gh_ingest_counts": (_int, [vp, _P(i64), _P(i64), _P(i64)]),
    "gh_ingest_chunking": (_int, [vp, _P(i64), _P(i64)]),
    "gh_ingest_copy_vertices": (_int, [vp, vp]),
    "gh_ingest_copy_edges": (_int, [vp, i32, vp]),
}
SYMBOLS = list(SIGNATURES)

_lib = None


def load():
    """Load the shared library (does not touch the GPU)."""
    global _lib
    if _lib is not None:
        return _lib
    global LIB_PATH
    if os.environ.get("GRAPHEM_HIP_LIB"):   # A/B runs against another build of the same library
        LIB_PATH = os.environ["GRAPHEM_HIP_LIB"]
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python graphem-rapids_amd/build.py` "
            "(hipcc --offload-arch=gfx950). The HIP backend has no CPU fallback.")
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def raise_for(status, handle, last_error="gh_last_error"):
    """Map a gh_status to the exception type the reference raises for the same condition; the message is the handle's, or
    with no handle the create-time message of the module whose `last_error` symbol is named."""
    if status == GH_OK:
        return
    msg = getattr(load(), last_error)(handle)
    msg = msg.decode() if msg else f"gh_status {status}"
    raise {GH_ERR_INVALID: ValueError, GH_ERR_NOMEM: MemoryError}.get(status, RuntimeError)(msg)


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class Handle:
    """Owner of one native handle.  A subclass names its module's symbols and opens the handle with _create."""
    _destroy = _last_error = None

    def _create(self, symbol, *args):
        """handle = symbol(&handle, *args); a failed create raises the module's create-time message and owns nothing."""
        self.lib = load()
        self.handle = ctypes.c_void_p()
        st = getattr(self.lib, symbol)(ctypes.byref(self.handle), *args)
        if st != GH_OK:
            self.handle = ctypes.c_void_p()
            self._raise(st)

    def _raise(self, st):
        if st != GH_OK:
            raise_for(st, self.handle if self.handle.value else None, self._last_error)

    _chk = _raise

    def close(self):
        if getattr(self, "handle", None) and self.handle.value:
            getattr(self.lib, self._destroy)(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # pylint: disable=broad-exception-caught
            pass


class BudgetHandle(Handle):
    """A handle whose calls size their working state by a memory budget (the default is in each class's docstring)."""
    _set_budget = None

    def set_memory_budget(self, nbytes):
        """Bytes of working state a call on this handle may hold (0: the module's default); results do not depend on it."""
        self._raise(getattr(self.lib, self._set_budget)(self.handle, int(nbytes)))


class Engine(Handle):
    """Thin RAII wrapper over a gh_handle."""
    _destroy, _last_error = "gh_destroy", "gh_last_error"

    def __init__(self, n, D, edges, L_min, k_attr, k_inter, n_neighbors, sample_size, seed=0, device_id=0,
                 partition=None, reorder="auto", knn_method="auto", knn_distance="exact", dtype="float32", ivf_lists=0,
                 ivf_probes=0):
        """dtype='float64': the engine of csrc/f64.hip -- every phase in double; positions, spring and intersection forces
        cross the boundary as float64 arrays (whole graph only; reorder / knn_method / knn_distance do not apply)."""
        self.n, self.D = int(n), int(D)
        if dtype not in ("float32", "float64"):
            raise ValueError(f"dtype must be 'float32' or 'float64', got {dtype!r}")
        self.f64 = dtype == "float64"
        self.np_dtype = np.float64 if self.f64 else np.float32
        if self.f64 and partition is not None:
            raise ValueError("the float64 engine takes the whole graph (no partition)")
        edges = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 2)
        self.E = edges.shape[0]
        prm = GhParams(float(L_min), float(k_attr), float(k_inter), int(n_neighbors), int(sample_size),
                       int(seed) & 0xFFFFFFFFFFFFFFFF, REORDER[reorder], KNN_METHOD[knn_method], KNN_DISTANCE[knn_distance],
                       int(ivf_lists), int(ivf_probes))
        part = None
        if partition is not None:
            vals = [int(x) for x in partition]  # (row_lo, row_hi, edge_lo, edge_hi[, edge_rule])
            part = ctypes.pointer(GhPartition(*(vals + [EDGES_RANGE] * (5 - len(vals)))))
        if self.f64:
            self._create("gh_create_f64", int(device_id), self.n, self.D, self.E, ptr(edges), ctypes.byref(prm), float(L_min),
                         float(k_attr), float(k_inter))
        else:
            self._create("gh_create", int(device_id), self.n, self.D, self.E, ptr(edges), ctypes.byref(prm), part)
        self.k = int(n_neighbors)
        self.S = min(int(sample_size), self.E)
        self.ld = self.lib.gh_row_stride(self.handle)

    def set_positions(self, pos):
        pos = np.ascontiguousarray(pos, dtype=self.np_dtype)
        if pos.shape != (self.n, self.D):
            raise ValueError(f"positions must have shape {(self.n, self.D)}, got {pos.shape}")
        self._chk((self.lib.gh_set_positions_f64 if self.f64 else self.lib.gh_set_positions)(self.handle, ptr(pos)))

    def get_positions(self):
        out = np.empty((self.n, self.D), dtype=self.np_dtype)
        self._chk((self.lib.gh_get_positions_f64 if self.f64 else self.lib.gh_get_positions)(self.handle, ptr(out)))
        return out

    def _ids(self, sampled):
        if sampled is None:
            return None
        sampled = np.ascontiguousarray(sampled, dtype=np.int32).ravel()
        if self.S < self.E and sampled.shape[0] != self.S:
            raise ValueError(f"expected {self.S} sampled edge ids, got {sampled.shape[0]}")
        return sampled

    def step(self, sampled=None):
        s = self._ids(sampled)
        self._chk(self.lib.gh_step(self.handle, ptr(s)))

    def run(self, iters, sample_stream=None):
        ss = None
        if sample_stream is not None:
            ss = np.ascontiguousarray(sample_stream, dtype=np.int32)
            if self.S < self.E and ss.shape != (iters, self.S):
                raise ValueError(f"sample_stream must have shape {(iters, self.S)}, got {ss.shape}")
        self._chk(self.lib.gh_run(self.handle, int(iters), ptr(ss)))

    def run_torch_sampled(self, iters, rng_state):
        """gh_run_torch_sampled: rng_state = uint8 array of torch.get_rng_state() (5056 bytes), updated in place."""
        if rng_state.dtype != np.uint8 or not rng_state.flags.c_contiguous or not rng_state.flags.writeable:
            raise ValueError("rng_state must be a writable contiguous uint8 array")
        self._chk(self.lib.gh_run_torch_sampled(self.handle, int(iters), ptr(rng_state), rng_state.size))

    def sampler_stats(self):
        """Host ms of the last run_torch_sampled: producer drawing, caller waiting for an upload slot, caller waiting for ids, the call."""
        out = np.zeros(4, dtype=np.float64)
        self._chk(self.lib.gh_sampler_stats(self.handle, ptr(out)))
        return {"draw_ms": out[0], "slot_wait_ms": out[1], "caller_wait_ms": out[2], "call_ms": out[3]}

    def sync(self):
        self._chk(self.lib.gh_sync(self.handle))

    def spring_forces(self):
        F = np.empty((self.n, self.D), dtype=self.np_dtype)
        self._chk((self.lib.gh_spring_forces_f64 if self.f64 else self.lib.gh_spring_forces)(self.handle, ptr(F)))
        return F

    def knn_midpoints(self, sampled=None):
        s = self._ids(sampled)
        knn = np.empty((self.S, self.k), dtype=np.int32)
        self._chk(self.lib.gh_knn_midpoints(self.handle, ptr(s), ptr(knn)))
        return knn

    def intersection_forces(self, sampled, knn):
        s = self._ids(sampled)
        knn = np.ascontiguousarray(knn, dtype=np.int32)
        if knn.shape != (self.S, self.k):
            raise ValueError(f"knn must have shape {(self.S, self.k)}, got {knn.shape}")
        F = np.empty((self.n, self.D), dtype=self.np_dtype)
        self._chk((self.lib.gh_intersection_forces_f64 if self.f64 else self.lib.gh_intersection_forces)(self.handle, ptr(s), ptr(knn), ptr(F)))
        return F

    def integrate_normalise(self, Fs, Fi):
        Fs = np.ascontiguousarray(Fs, dtype=np.float32)
        Fi = np.ascontiguousarray(Fi, dtype=np.float32)
        if Fs.shape != (self.n, self.D) or Fi.shape != (self.n, self.D):
            raise ValueError("force arrays must have the shape of positions")
        out = np.empty((self.n, self.D), dtype=np.float32)
        self._chk(self.lib.gh_integrate_normalise(self.handle, ptr(Fs), ptr(Fi), ptr(out)))
        return out

    # multi-GPU split step
    def step_begin(self, sampled=None):
        s = self._ids(sampled)
        self._chk(self.lib.gh_step_begin(self.handle, ptr(s)))

    def step_merge(self, gathered_ptr, world):
        self._chk(self.lib.gh_step_merge(self.handle, ctypes.c_void_p(gathered_ptr), int(world)))

    def step_finish(self):
        self._chk(self.lib.gh_step_finish(self.handle))

    def set_stream(self, stream_ptr, use_own=False):
        """Enqueue on the given raw HIP stream (0 = the default stream) or back on the engine's own."""
        self._chk(self.lib.gh_set_stream(self.handle, ctypes.c_void_p(stream_ptr), 1 if use_own else 0))

    def positions_rows_allocated(self):
        return int(self.lib.gh_positions_rows_allocated(self.handle))

    def stats_rows(self):
        return int(self.lib.gh_stats_rows(self.handle))

    def radial_topk(self, k):
        """The k vertices farthest from the origin, farthest first (include/graphem_hip.h gh_radial_topk)."""
        out = np.empty(int(k), dtype=np.int32)
        self._chk(self.lib.gh_radial_topk(self.handle, int(k), ptr(out)))
        return out

    def vertex_order(self):
        """order[v] = row of vertex v in the device position array."""
        out = np.empty(self.n, dtype=np.int32)
        self._chk(self.lib.gh_vertex_order(self.handle, ptr(out)))
        return out

    def positions_unpadded_device_ptr(self):
        p = self.lib.gh_positions_unpadded_device(self.handle)
        if not p:
            raise RuntimeError("gh_positions_unpadded_device failed")
        return p

    def gather_layout(self, world, rank, chunk):
        self._chk(self.lib.gh_gather_layout(self.handle, int(world), int(rank), int(chunk)))

    def rank_layout(self, world, rank, chunk):
        self._chk(self.lib.gh_rank_layout(self.handle, int(world), int(rank), int(chunk)))

    # form D (include/graphem_hip.h gh_overlap_layout)
    def overlap_layout(self, world, rank, chunk):
        self._chk(self.lib.gh_overlap_layout(self.handle, int(world), int(rank), int(chunk)))

    def rows_all_device_ptr(self):
        return self.lib.gh_rows_all_device(self.handle)

    def rows_all_row_floats(self):
        return int(self.lib.gh_rows_all_row_floats(self.handle))

    def stats_all_device_ptr(self):
        return self.lib.gh_stats_all_device(self.handle)

    def stats_all_block_doubles(self):
        return int(self.lib.gh_stats_all_block_doubles(self.handle))

    def step_rows_early(self):
        return bool(self.lib.gh_step_rows_early(self.handle))

    def step_pack_rows(self, stream_ptr=None):
        """Own block of new0 -> its packed slot, on the given raw HIP stream (None: the engine's stream)."""
        self._chk(self.lib.gh_step_pack_rows(self.handle, ctypes.c_void_p(stream_ptr or 0), 1 if stream_ptr is None else 0))

    def step_finish_overlap(self):
        self._chk(self.lib.gh_step_finish_overlap(self.handle))

    def step_finish_own(self, stats_all_ptr, world):
        self._chk(self.lib.gh_step_finish_own(self.handle, ctypes.c_void_p(stats_all_ptr), int(world)))

    def rows_packed_device_ptr(self):
        """(world, chunk, D) float32: the finished blocks without pad columns (0 when D == ld or world == 1)."""
        return self.lib.gh_rows_packed_device(self.handle)

    def step_unpack_rows(self):
        self._chk(self.lib.gh_step_unpack_rows(self.handle))

    def set_packed_rows(self, on):
        """Finished blocks travel without pad columns + expansion kernel (default: from 2 M vertices on)."""
        self._chk(self.lib.gh_set_packed_rows(self.handle, 1 if on else 0))

    def gather_buffer_device_ptr(self):
        return self.lib.gh_gather_buffer_device(self.handle)

    def gather_slot_bytes(self):
        return int(self.lib.gh_gather_slot_bytes(self.handle))

    def step_finish_gathered(self):
        self._chk(self.lib.gh_step_finish_gathered(self.handle))

    # the whole partitioned run in one call (csrc/comm.hip)
    def comm_init_rccl(self, world, rank, unique_id):
        """unique_id: the 128 bytes rank 0 got from comm_unique_id(), the same on every rank."""
        buf = ctypes.create_string_buffer(bytes(unique_id), 128)
        self._chk(self.lib.gh_comm_init_rccl(self.handle, int(world), int(rank), ctypes.cast(buf, ctypes.c_void_p)))

    def comm_init_loopback(self, group, rank):
        self._chk(self.lib.gh_comm_init_loopback(self.handle, group, int(rank)))

    def comm_destroy(self):
        self._chk(self.lib.gh_comm_destroy(self.handle))

    def run_partitioned(self, iters, sample_stream=None):
        ss = None
        if sample_stream is not None:
            ss = np.ascontiguousarray(sample_stream, dtype=np.int32)
            if self.S < self.E and ss.shape != (iters, self.S):
                raise ValueError(f"sample_stream must have shape {(iters, self.S)}, got {ss.shape}")
        self._chk(self.lib.gh_run_partitioned(self.handle, int(iters), ptr(ss)))

    def positions_device_ptr(self):
        return (self.lib.gh_positions_device_f64 if self.f64 else self.lib.gh_positions_device)(self.handle)

    def knn_partial_device_ptr(self):
        return self.lib.gh_knn_partial_device(self.handle)

    def knn_merged_device_ptr(self):
        """(S, k + 1) keys of the global KNN after step_merge (0 before the first merge)."""
        return self.lib.gh_knn_merged_device(self.handle)

    def knn_partial_cols(self):
        """64-bit words per query of the record a rank sends after part 1 of a split step: k + 1 keys; a
        knn_distance='cdist' engine on a row partition sends k + 2 keys and a flag (include/graphem_hip.h)."""
        return int(self.lib.gh_knn_partial_cols(self.handle))

    def stats_partial_device_ptr(self):
        return self.lib.gh_stats_partial_device(self.handle)

    def knn_last_counts(self):
        """(subset_counts, final_counts, overflow) of the last KNN search, each (S,) int32."""
        a, b, c = (np.zeros(self.S, dtype=np.int32) for _ in range(3))
        self._chk(self.lib.gh_knn_last_counts(self.handle, ptr(a), ptr(b), ptr(c)))
        return a, b, c

    def knn_cdist_stats(self):
        """(rows that took the pass over all edges, rows with a tie ATen's nth_element path decides) of the last
        KNN search of a knn_distance='cdist' engine."""
        a, b = ctypes.c_int32(0), ctypes.c_int32(0)
        self._chk(self.lib.gh_knn_cdist_stats(self.handle, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def set_cdist_replay(self, all_ties):
        """The loop of a knn_distance='cdist' engine replays every tie (True) or only those that can change a force (False, default)."""
        self._chk(self.lib.gh_set_cdist_replay(self.handle, 1 if all_ties else 0))

    def set_scan_filter(self, mode):
        """Pre-filter of the fused kernel for n_components <= 3: 'auto', 'mfma' or 'cells' (same results either way)."""
        self._chk(self.lib.gh_set_scan_filter(self.handle, SCAN_FILTERS[mode]))

    def scan_filter(self):
        """The pre-filter in use: 'cells', 'mfma', or 'auto' when the engine runs neither."""
        v = ctypes.c_int32(0)
        self._chk(self.lib.gh_get_scan_filter(self.handle, ctypes.byref(v)))
        return {b: a for a, b in SCAN_FILTERS.items()}[v.value]

    def set_coarse_tau(self, mode):
        """Thresholds of the query-cell filter: 'on' = from 64 coarse group minima inside the fused launch, 'off' = a launch
        of their own, 'auto' (same results either way)."""
        self._chk(self.lib.gh_set_coarse_tau(self.handle, COARSE_TAU[mode]))

    def coarse_tau(self):
        """True when the fused launch computes the thresholds itself from the coarse table."""
        v = ctypes.c_int32(0)
        self._chk(self.lib.gh_get_coarse_tau(self.handle, ctypes.byref(v)))
        return bool(v.value)

    def set_compact_gather(self, mode):
        """Position rows of the three-component fused kernel: 'on' = from the table of 12-byte rows packed five to a 64-byte
        sector, 'off' = from the padded positions, 'auto' (same results either way)."""
        self._chk(self.lib.gh_set_compact_gather(self.handle, COMPACT_GATHER[mode]))

    def compact_gather(self):
        """True when the engine keeps the sector-packed table and its fused kernel reads it."""
        v = ctypes.c_int32(0)
        self._chk(self.lib.gh_get_compact_gather(self.handle, ctypes.byref(v)))
        return bool(v.value)

    def compact_gather_launches(self):
        """Fused launches of this engine so far that read the sector-packed table (the others read the padded positions)."""
        v = ctypes.c_int64(0)
        self._chk(self.lib.gh_compact_gather_launches(self.handle, ctypes.byref(v)))
        return v.value

    def coarse_table(self):
        """Both copies of the coarse table as (2, 64, sample_size) uint32 float bits; 0xFFFFFFFF = empty (diagnostic)."""
        out = np.empty((2, COARSE_GROUPS, self.S), dtype=np.uint32)
        self._chk(self.lib.gh_debug_coarse_table(self.handle, out.ctypes.data_as(ctypes.c_void_p), out.size))
        return out

    def knn_ivf_config(self):
        """(lists, probes per query) of a knn_method='ivf' engine; (0, 0) otherwise."""
        a, b = ctypes.c_int32(0), ctypes.c_int32(0)
        self._chk(self.lib.gh_knn_ivf_config(self.handle, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def knn_ivf_list_sizes(self):
        """(lists,) int32 members of every inverted list after the last search."""
        out = np.zeros(self.knn_ivf_config()[0], dtype=np.int32)
        self._chk(self.lib.gh_knn_ivf_list_sizes(self.handle, ptr(out), len(out)))
        return out

    # instrumentation
    def timing_enable(self, on=True):
        self._chk(self.lib.gh_timing_enable(self.handle, 1 if on else 0))

    def timing_reset(self):
        self._chk(self.lib.gh_timing_reset(self.handle))

    def timings(self):
        """{kernel name: (total_ms, launches)} since the last reset."""
        out = {}
        for i in range(self.lib.gh_timing_count(self.handle)):
            name, ms, cnt = ctypes.c_char_p(), ctypes.c_double(), ctypes.c_int64()
            self._chk(self.lib.gh_timing_get(self.handle, i, ctypes.byref(name), ctypes.byref(ms), ctypes.byref(cnt)))
            out[name.value.decode()] = (ms.value, cnt.value)
        return out


LT = "lt"   # what ICGraph.spread / rr_sample take as p for the handle's Linear Threshold table


class ICGraph(BudgetHandle):
    """Thin RAII wrapper over a gh_ic_handle: Monte Carlo Independent Cascade on one graph (include/graphem_hip.h).
    Memory budget: device bytes of chunk state a spread call may hold, 1 GiB by default."""
    _destroy, _last_error, _set_budget = "gh_ic_destroy", "gh_ic_last_error", "gh_ic_set_memory_budget"

    def __init__(self, n, arcs, directed=False, device_id=0):
        self.n, self.directed = int(n), bool(directed)
        arcs = np.ascontiguousarray(arcs, dtype=np.int32).reshape(-1, 2)
        self._create("gh_ic_create", int(device_id), self.n, arcs.shape[0], ptr(arcs), 1 if self.directed else 0)
        self.arcs = int(self.lib.gh_ic_arc_count(self.handle))

    def set_arc_probabilities(self, pairs, prob):
        """The handle's per-arc table (gh_ic_set_arc_probabilities): pairs (m, 2) directed u -> v, prob (m,) float64.  Arcs
        that are not listed get probability 0; a failed call keeps the previous table."""
        pairs = np.asarray(pairs).reshape(-1, 2)
        prob = np.ascontiguousarray(np.asarray(prob).ravel(), dtype=np.float64)
        if len(prob) != len(pairs):
            raise ValueError(f"{len(pairs)} pairs but {len(prob)} probabilities")
        if len(pairs) and (pairs.min() < 0 or pairs.max() >= self.n):   # before the cast to int32 can wrap an id
            raise ValueError(f"pair endpoints must lie in [0, {self.n})")
        pairs = np.ascontiguousarray(pairs, dtype=np.int32)
        self._raise(self.lib.gh_ic_set_arc_probabilities(self.handle, len(pairs), ptr(pairs), ptr(prob)))

    def set_lt_weights(self, pairs, weight):
        """The handle's Linear Threshold table (gh_ic_set_lt_weights): pairs (m, 2) directed u -> v, weight (m,) float64.
        Arcs that are not listed get weight 0; a failed call keeps the previous table.  The per-arc table is another one."""
        pairs = np.asarray(pairs).reshape(-1, 2)
        weight = np.ascontiguousarray(np.asarray(weight).ravel(), dtype=np.float64)
        if len(weight) != len(pairs):
            raise ValueError(f"{len(pairs)} pairs but {len(weight)} weights")
        if len(pairs) and (pairs.min() < 0 or pairs.max() >= self.n):   # before the cast to int32 can wrap an id
            raise ValueError(f"pair endpoints must lie in [0, {self.n})")
        pairs = np.ascontiguousarray(pairs, dtype=np.int32)
        self._raise(self.lib.gh_ic_set_lt_weights(self.handle, len(pairs), ptr(pairs), ptr(weight)))

    def spread(self, sets, p, n_trials, seed=0, max_hops=-1, base=None, per_trial=False):
        """sets: a list of vertex-id sequences.  Returns totals (n_sets,) int64 and, with per_trial, the (n_sets, n_trials)
        int32 counts; with a base set both are marginal over it (gh_ic_spread; p=None: the handle's per-arc table,
        gh_ic_spread_arcs; p=LT: its Linear Threshold table, gh_ic_spread_lt)."""
        sets = [np.asarray(s, dtype=np.int64).ravel() for s in sets]
        offsets = np.zeros(len(sets) + 1, dtype=np.int64)
        offsets[1:] = np.cumsum([len(s) for s in sets])
        verts = np.ascontiguousarray(np.concatenate(sets) if sets else np.zeros(0), dtype=np.int32)
        base = np.ascontiguousarray(np.zeros(0) if base is None else np.asarray(base).ravel(), dtype=np.int32)
        totals = np.zeros(len(sets), dtype=np.int64)
        trials = np.zeros((len(sets), int(n_trials)), dtype=np.int32) if per_trial else None
        rest = (int(max_hops), int(n_trials), int(seed) & 0xFFFFFFFFFFFFFFFF, len(sets), ptr(offsets), ptr(verts), ptr(base),
                len(base), ptr(totals), ptr(trials))
        self._raise(self.lib.gh_ic_spread_lt(self.handle, *rest) if (isinstance(p, str) and p == LT) else
                    self.lib.gh_ic_spread_arcs(self.handle, *rest) if p is None else
                    self.lib.gh_ic_spread(self.handle, float(p), *rest))
        return (totals, trials) if per_trial else totals


    def rr_sample(self, rr, n_samples, p, seed=0, max_hops=-1, trials=None, roots=None):
        """Appends n_samples reverse-reachable sets to the RRSets `rr` (gh_ic_rr_sample); trials uint64 / roots int32 of
        n_samples, or None for the header's defaults.  p=None: the handle's per-arc table (gh_ic_rr_sample_arcs); p=LT: its
        Linear Threshold table (gh_ic_rr_sample_lt)."""
        n_samples = int(n_samples)
        if trials is not None:
            trials = np.ascontiguousarray(np.asarray(trials).ravel(), dtype=np.uint64)
        if roots is not None:
            roots = np.ascontiguousarray(np.asarray(roots).ravel(), dtype=np.int32)
        for a in (trials, roots):
            if a is not None and len(a) != n_samples:
                raise ValueError(f"trials and roots must have n_samples = {n_samples} entries")
        rest = (int(max_hops), int(seed) & 0xFFFFFFFFFFFFFFFF, n_samples, ptr(trials), ptr(roots))
        self._raise(self.lib.gh_ic_rr_sample_lt(self.handle, rr.handle, *rest) if (isinstance(p, str) and p == LT) else
                    self.lib.gh_ic_rr_sample_arcs(self.handle, rr.handle, *rest) if p is None else
                    self.lib.gh_ic_rr_sample(self.handle, rr.handle, float(p), *rest))


class RRSets(BudgetHandle):
    """Thin RAII wrapper over a gh_rr_handle: a collection of reverse-reachable sets (or any set system over 0 .. n-1) on
    the device (include/graphem_hip.h).  Memory budget: device bytes the collection may hold, 4 GiB by default."""
    _destroy, _last_error, _set_budget = "gh_rr_destroy", "gh_rr_last_error", "gh_rr_set_memory_budget"

    def __init__(self, n, device_id=0):
        self.n = int(n)
        self._create("gh_rr_create", int(device_id), self.n)

    def counts(self):
        """(sets, members in all)."""
        sets, members = ctypes.c_int64(), ctypes.c_int64()
        self._raise(self.lib.gh_rr_counts(self.handle, ctypes.byref(sets), ctypes.byref(members)))
        return sets.value, members.value

    def download(self):
        """(indptr int64 (sets + 1), members int32, roots int32 (sets))."""
        sets, total = self.counts()
        indptr, members, roots = np.zeros(sets + 1, dtype=np.int64), np.zeros(total, dtype=np.int32), np.zeros(sets, dtype=np.int32)
        self._raise(self.lib.gh_rr_download(self.handle, ptr(indptr), ptr(members), ptr(roots)))
        return indptr, members, roots

    def upload(self, indptr, members, roots=None):
        indptr = np.ascontiguousarray(np.asarray(indptr).ravel(), dtype=np.int64)
        members = np.ascontiguousarray(np.asarray(members).ravel(), dtype=np.int32)
        if len(indptr) < 1 or (len(indptr) > 0 and indptr[-1] != len(members)):
            raise ValueError("indptr must have sets + 1 entries and end at len(members)")
        if roots is not None:
            roots = np.ascontiguousarray(np.asarray(roots).ravel(), dtype=np.int32)
            if len(roots) != len(indptr) - 1:
                raise ValueError("roots must have one entry per set")
        self._raise(self.lib.gh_rr_upload(self.handle, len(indptr) - 1, ptr(indptr), ptr(members), ptr(roots)))

    def cover(self, k):
        """Greedy maximum coverage: (seeds int32, gains int64) of min(k, n) rounds (gh_rr_cover)."""
        rounds = max(0, min(int(k), self.n))
        seeds, gains = np.zeros(rounds, dtype=np.int32), np.zeros(rounds, dtype=np.int64)
        self._raise(self.lib.gh_rr_cover(self.handle, int(k), ptr(seeds), ptr(gains)))
        return seeds, gains

    def count_hit(self, vertices):
        verts = np.ascontiguousarray(np.asarray(vertices).ravel(), dtype=np.int32)
        count = ctypes.c_int64()
        self._raise(self.lib.gh_rr_count_hit(self.handle, ptr(verts), len(verts), ctypes.byref(count)))
        return count.value


class CentGraph(BudgetHandle):
    """Thin RAII wrapper over a gh_cent_handle: shortest-path centralities, PageRank, the adjacency SpMV, graph statistics
    and communities of one undirected graph (include/graphem_hip.h).  Memory budget: device bytes of path state a paths
    call (or of spill tables a louvain call) may hold, 1 GiB by default."""
    _destroy, _last_error, _set_budget = "gh_cent_destroy", "gh_cent_last_error", "gh_cent_set_memory_budget"

    def __init__(self, n, edges, device_id=0):
        self.n = int(n)
        edges = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 2)
        self._create("gh_cent_create", int(device_id), self.n, edges.shape[0], ptr(edges))
        self.edges = int(self.lib.gh_cent_edge_count(self.handle))

    def paths(self, sources, betweenness=True, load=True, distances=True):
        """One all-sources pass (gh_cent_paths): (betweenness (n,), load (n,), reached (S,), dist_sum (S,)); a part not
        asked for is None.  Raw sums, unnormalised."""
        src = np.ascontiguousarray(np.asarray(sources, dtype=np.int64).ravel())
        if len(src) and (src.min() < 0 or src.max() >= self.n):
            raise ValueError(f"source ids must lie in [0, {self.n})")
        src = src.astype(np.int32)
        bc = np.zeros(self.n) if betweenness else None
        ld = np.zeros(self.n) if load else None
        reached = np.zeros(len(src), dtype=np.int64) if distances else None
        dsum = np.zeros(len(src), dtype=np.int64) if distances else None
        self._raise(self.lib.gh_cent_paths(self.handle, len(src), ptr(src), ptr(bc), ptr(ld), ptr(reached), ptr(dsum)))
        return bc, ld, reached, dsum

    def pagerank(self, alpha, max_iter, tol):
        """(x (n,), iterations): iterations = -1 when max_iter iterations did not converge (gh_cent_pagerank)."""
        x = np.zeros(self.n)
        its = ctypes.c_int32(0)
        self._raise(self.lib.gh_cent_pagerank(self.handle, float(alpha), int(max_iter), float(tol), ptr(x), ctypes.byref(its)))
        return x, int(its.value)

    def components(self):
        """(labels (n,) int32, n_components): labels[v] = the smallest vertex id in v's component (gh_cent_components)."""
        labels = np.zeros(self.n, dtype=np.int32)
        count = ctypes.c_int64(0)
        self._raise(self.lib.gh_cent_components(self.handle, ptr(labels), ctypes.byref(count)))
        return labels, int(count.value)

    def distances(self, sources, reached=True, dist_sum=True, eccentricity=True):
        """Breadth-first levels from `sources` (gh_cent_distances): (reached (S,) int64, dist_sum (S,) int64, eccentricity
        (S,) int32); a part not asked for is None."""
        src = np.ascontiguousarray(np.asarray(sources, dtype=np.int64).ravel())
        if len(src) and (src.min() < 0 or src.max() >= self.n):
            raise ValueError(f"source ids must lie in [0, {self.n})")
        src = src.astype(np.int32)
        cnt = np.zeros(len(src), dtype=np.int64) if reached else None
        dsum = np.zeros(len(src), dtype=np.int64) if dist_sum else None
        ecc = np.zeros(len(src), dtype=np.int32) if eccentricity else None
        self._raise(self.lib.gh_cent_distances(self.handle, len(src), ptr(src), ptr(cnt), ptr(dsum), ptr(ecc)))
        return cnt, dsum, ecc

    def triangles(self):
        """(n,) int64 triangles through every vertex (gh_cent_triangles)."""
        tri = np.zeros(self.n, dtype=np.int64)
        self._raise(self.lib.gh_cent_triangles(self.handle, ptr(tri)))
        return tri

    def cores(self):
        """(core (n,) int32, layer (n,) int32, rounds): core numbers, onion layers and the number of peel rounds
        (gh_cent_cores)."""
        core = np.zeros(self.n, dtype=np.int32)
        layer = np.zeros(self.n, dtype=np.int32)
        rounds = ctypes.c_int32(0)
        self._raise(self.lib.gh_cent_cores(self.handle, ptr(core), ptr(layer), ctypes.byref(rounds)))
        return core, layer, int(rounds.value)

    def truss(self):
        """(truss (edges,) int32 in canonical edge order, rounds) (gh_cent_truss)."""
        truss = np.zeros(self.edges, dtype=np.int32)
        rounds = ctypes.c_int32(0)
        self._raise(self.lib.gh_cent_truss(self.handle, ptr(truss), ctypes.byref(rounds)))
        return truss, int(rounds.value)

    def link_scores(self, pairs, cn=True, aa=True, ra=True):
        """(cn, aa, ra), (P,) int64 each, of the vertex pairs `pairs` ((P, 2) ids; gh_cent_link_scores): common
        neighbours and the fixed-point Adamic-Adar and resource-allocation sums (scale 2^32); a part not asked for is None."""
        pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        if len(pairs) and (pairs.min() < 0 or pairs.max() >= self.n):
            raise ValueError(f"vertex ids must lie in [0, {self.n})")
        pairs = np.ascontiguousarray(pairs, dtype=np.int32)
        out = [np.zeros(len(pairs), dtype=np.int64) if want else None for want in (cn, aa, ra)]
        self._raise(self.lib.gh_cent_link_scores(self.handle, len(pairs), ptr(pairs), ptr(out[0]), ptr(out[1]), ptr(out[2])))
        return tuple(out)

    def link_candidates(self, kind, k, rows):
        """(ids (R, k) int32, num (R, k) int64, den (R, k) int64): the k best two-hop candidates of every source in `rows`
        under score kind `kind` (a LINK_KINDS name or code), best first; unused slots hold -1, 0, 1
        (gh_cent_link_candidates)."""
        kind = LINK_KINDS[kind] if isinstance(kind, str) else int(kind)
        k = int(k)
        if not 1 <= k <= LINK_MAX_K:
            raise ValueError(f"k must lie in [1, {LINK_MAX_K}]")
        rows = np.asarray(rows, dtype=np.int64).ravel()
        if len(rows) and (rows.min() < 0 or rows.max() >= self.n):
            raise ValueError(f"vertex ids must lie in [0, {self.n})")
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        ids = np.full((len(rows), k), -1, dtype=np.int32)
        num = np.zeros((len(rows), k), dtype=np.int64)
        den = np.ones((len(rows), k), dtype=np.int64)
        self._raise(self.lib.gh_cent_link_candidates(self.handle, kind, k, len(rows), ptr(rows), ptr(ids), ptr(num), ptr(den)))
        return ids, num, den

    def label_propagation(self, seed_labels, n_classes, max_rounds=100):
        """(labels (n,) int32, rounds, converged): synchronous label propagation from the seeds (gh_cent_label_propagation).
        seed_labels: n entries, -1 = unlabelled, else a class in [0, n_classes); seeds never change."""
        seed_labels = np.asarray(seed_labels).ravel()
        if len(seed_labels) != self.n:
            raise ValueError(f"{len(seed_labels)} seed labels for {self.n} vertices")
        seed_labels = np.ascontiguousarray(np.clip(seed_labels, -2, LABEL_MAX_CLASSES), dtype=np.int32)   # out of range stays so
        labels = np.zeros(self.n, dtype=np.int32)
        rounds, converged = ctypes.c_int32(), ctypes.c_int32()
        self._raise(self.lib.gh_cent_label_propagation(self.handle, int(n_classes), ptr(seed_labels), int(max_rounds), ptr(labels),
                                                       ctypes.byref(rounds), ctypes.byref(converged)))
        return labels, int(rounds.value), bool(converged.value)

    def modularity(self, labels):
        """(sum I, sum T^2, M) of a labelling with values in [0, n), as Python ints (gh_cent_modularity)."""
        labels = np.ascontiguousarray(labels, dtype=np.int32).ravel()
        if len(labels) != self.n:
            raise ValueError(f"labels must have {self.n} entries")
        out = np.zeros(3, dtype=np.int64)
        self._raise(self.lib.gh_cent_modularity(self.handle, ptr(labels), ptr(out)))
        return int(out[0]), int(out[1]), int(out[2])

    def louvain(self, seed=0, max_levels=32, max_rounds=1000):
        """The Louvain levels (gh_cent_louvain): (labels (L, n) int32, numerators [L] of Python ints, n_communities (L,)
        int64, rounds (L,) int32, M)."""
        max_levels = int(max_levels)
        if max_levels < 1 or int(max_rounds) < 1:
            raise ValueError("max_levels and max_rounds must be >= 1")
        labels = np.zeros((max_levels, self.n), dtype=np.int32)
        numerators = np.zeros(max_levels, dtype=np.int64)
        counts = np.zeros(max_levels, dtype=np.int64)
        rounds = np.zeros(max_levels, dtype=np.int32)
        levels = ctypes.c_int32(0)
        self._raise(self.lib.gh_cent_louvain(self.handle, int(seed) & 0xFFFFFFFFFFFFFFFF, max_levels, int(max_rounds), ptr(labels),
                                             ctypes.byref(levels), ptr(numerators), ptr(counts), ptr(rounds)))
        L = int(levels.value)
        return labels[:L].copy(), [int(x) for x in numerators[:L]], counts[:L].copy(), rounds[:L].copy(), 2 * self.edges

    def csr_device(self):
        """(indptr, indices) device pointers of the handle's symmetric CSR."""
        ip, ix = ctypes.c_void_p(), ctypes.c_void_p()
        self._raise(self.lib.gh_cent_csr_device(self.handle, ctypes.byref(ip), ctypes.byref(ix)))
        return ip.value, ix.value

    def spmv_shift(self, stream, x_ptr, y_ptr, c):
        """y = A x + c x on device pointers, enqueued on `stream` (gh_spmv_adj_shift)."""
        ip, ix = self.csr_device()
        st = self.lib.gh_spmv_adj_shift(ctypes.c_void_p(stream), self.n, ctypes.c_void_p(ip), ctypes.c_void_p(ix), float(c),
                                        ctypes.c_void_p(x_ptr), ctypes.c_void_p(y_ptr))
        if st != GH_OK:
            msg = self.lib.gh_cent_last_error(None)
            raise RuntimeError(msg.decode() if msg else f"gh_status {st}")


def link_weight(kind, degree):
    """The fixed-point weight (scale 2^32) a common neighbour of that degree adds to the sum of score `kind` (a LINK_KINDS
    name or code; gh_link_weight, no device)."""
    kind = LINK_KINDS[kind] if isinstance(kind, str) else int(kind)
    w = int(load().gh_link_weight(kind, int(degree)))
    if w < 0:
        raise ValueError(f"no link weight for kind {kind} and degree {degree}")
    return w


def knn_points(query, reference, k, device_id=0):
    """(n_query, k) int64 ids of the k nearest reference rows (gh_knn_points)."""
    query = np.ascontiguousarray(query, dtype=np.float32)
    reference = np.ascontiguousarray(reference, dtype=np.float32)
    if query.ndim != 2 or reference.ndim != 2 or query.shape[1] != reference.shape[1]:
        raise ValueError("query and reference must be 2-D with the same number of columns")
    out = np.empty((query.shape[0], int(k)), dtype=np.int64)
    st = load().gh_knn_points(int(device_id), ptr(query), query.shape[0], ptr(reference), reference.shape[0],
                              query.shape[1], int(k), ptr(out))
    raise_for(st, None)
    return out


def torch_randperm_prefix(rng_state, n, S, iters=1):
    """(iters, S) int32 = `iters` successive torch.randperm(n)[:S] of the CPU generator state in `rng_state` (uint8 array
    of torch.get_rng_state(), 5056 bytes), which is moved on in place exactly as those calls would (pure host code)."""
    if rng_state.dtype != np.uint8 or not rng_state.flags.c_contiguous or not rng_state.flags.writeable:
        raise ValueError("rng_state must be a writable contiguous uint8 array")
    out = np.empty((int(iters), int(S)), dtype=np.int32)
    st = load().gh_torch_randperm_prefix(ptr(rng_state), rng_state.size, int(n), int(S), int(iters), ptr(out))
    if st != GH_OK:
        raise ValueError("gh_torch_randperm_prefix: not a torch CPU generator state, or sizes out of range")
    return out


def torch_randperm_isa():
    return load().gh_torch_randperm_isa().decode()


def comm_unique_id():
    """128 bytes identifying a new RCCL communicator (ncclGetUniqueId); rank 0 makes it, every rank gets a copy."""
    buf = ctypes.create_string_buffer(128)
    st = load().gh_comm_unique_id(ctypes.cast(buf, ctypes.c_void_p))
    if st != GH_OK:
        raise RuntimeError(load().gh_comm_last_error().decode())
    return buf.raw


def comm_available():
    """True when librccl.so opens with every entry point the native loop uses (no communicator is made)."""
    return bool(load().gh_comm_available())


def selftest_arith(samples, seed=1, device_id=0):
    """(mismatches of the lean sqrt, of the lean division) against sqrtf and '/' on `samples` operand sets."""
    a, b = ctypes.c_int64(-1), ctypes.c_int64(-1)
    raise_for(load().gh_selftest_arith(int(device_id), int(seed), int(samples), ctypes.byref(a), ctypes.byref(b)), None)
    return a.value, b.value


def device_count():
    return int(load().gh_device_count())


def live_allocations():
    """(count, bytes) of the device allocations the library's handles hold in this process (gh_debug_live_allocations)."""
    count, nbytes = ctypes.c_int64(), ctypes.c_int64()
    load().gh_debug_live_allocations(ctypes.byref(count), ctypes.byref(nbytes))
    return count.value, nbytes.value


class Generator(BudgetHandle):
    """Thin RAII wrapper over a gh_gen_handle: the counter-based graph generators (include/graphem_hip.h).  device_id < 0
    is the library's host path, which touches no device and returns the same edges bit for bit.  Memory budget: bytes a call may allocate
    for counts and edges, 4 GiB by default; more is a MemoryError, never a cut."""
    _destroy, _last_error, _set_budget = "gh_gen_destroy", "gh_gen_last_error", "gh_gen_set_memory_budget"

    def __init__(self, device_id=0):
        self.device_id = int(device_id)
        self.rounds = 0
        self._create("gh_gen_create", self.device_id)

    def _edges(self, count):
        edges = np.zeros((int(count), 2), dtype=np.int32)
        self._raise(self.lib.gh_gen_edges(self.handle, ptr(edges)))
        return edges

    def sbm(self, sizes, p_matrix, seed=0):
        """(E, 2) int32 edges of the block model (gh_gen_sbm)."""
        sizes = np.ascontiguousarray(sizes, dtype=np.int64).ravel()
        P = np.ascontiguousarray(p_matrix, dtype=np.float64)
        if P.shape != (len(sizes), len(sizes)) and (len(sizes) or P.size):
            raise ValueError("p_matrix must be (blocks, blocks)")
        count = ctypes.c_int64()
        self._raise(self.lib.gh_gen_sbm(self.handle, len(sizes), ptr(sizes), ptr(P), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                        ctypes.byref(count)))
        return self._edges(count.value)

    def geometric(self, n, radius, dim=2, seed=0):
        """(edges (E, 2) int32, positions (n, dim) float32) of the random geometric graph (gh_gen_geometric)."""
        count = ctypes.c_int64()
        self._raise(self.lib.gh_gen_geometric(self.handle, int(n), float(radius), int(dim), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                              ctypes.byref(count)))
        pos = np.zeros((int(n), int(dim)), dtype=np.float32)
        self._raise(self.lib.gh_gen_positions(self.handle, ptr(pos)))
        return self._edges(count.value), pos

    def ba(self, n, m, seed=0):
        """(E, 2) int32 edges of the preferential-attachment graph (gh_gen_ba); self.rounds = launches it took."""
        count, rounds = ctypes.c_int64(), ctypes.c_int32()
        self._raise(self.lib.gh_gen_ba(self.handle, int(n), int(m), int(seed) & 0xFFFFFFFFFFFFFFFF, ctypes.byref(count),
                                       ctypes.byref(rounds)))
        self.rounds = int(rounds.value)
        return self._edges(count.value)


class Correlation(BudgetHandle):
    """Thin RAII wrapper over a gh_corr_handle: Spearman's rho between the columns of one table, plain and over bootstrap
    resamples (include/graphem_hip.h "rank correlation").  columns: (m, n) float64, one row per variable.  device_id < 0
    is the library's host path, which touches no device and returns the same integers bit for bit.  Memory budget: device bytes of
    replicate state a bootstrap call may hold, 4 GiB by default."""
    _destroy, _last_error, _set_budget = "gh_corr_destroy", "gh_corr_last_error", "gh_corr_set_memory_budget"

    def __init__(self, columns, device_id=0):
        self.device_id = int(device_id)
        cols = np.ascontiguousarray(columns, dtype=np.float64)
        if cols.ndim != 2:
            raise ValueError("columns must be (m, n)")
        self.m, self.n = int(cols.shape[0]), int(cols.shape[1])
        self._create("gh_corr_create", self.device_id, self.n, self.m, ptr(cols))

    def matrix(self, sums=False):
        """(m, m) float64 Spearman matrix of the plain statistic (gh_corr_matrix); with sums=True also the int64
        (m, m, 3) triples (Sxy, Sxx, Syy)."""
        out = np.zeros((self.m, self.m), dtype=np.float64)
        trip = np.zeros((self.m, self.m, 3), dtype=np.int64) if sums else None
        self._raise(self.lib.gh_corr_matrix(self.handle, ptr(out), ptr(trip)))
        return (out, trip) if sums else out

    def bootstrap(self, pairs, reps, seed=0, sums=False):
        """(n_pairs, reps) float64 rho of every pair of columns in every resample (gh_corr_bootstrap); with sums=True also
        the int64 (n_pairs, reps, 3) triples."""
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        reps = int(reps)
        shape = (len(pairs), max(reps, 0))
        out = np.zeros(shape, dtype=np.float64)
        trip = np.zeros(shape + (3,), dtype=np.int64) if sums else None
        self._raise(self.lib.gh_corr_bootstrap(self.handle, len(pairs), ptr(pairs), reps, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                               ptr(out), ptr(trip)))
        return (out, trip) if sums else out


def corr_rho(sxy, sxx, syy):
    """The library's conversion of a triple of sums to rho (gh_corr_rho)."""
    return float(load().gh_corr_rho(int(sxy), int(sxx), int(syy)))


class LayoutQuality(Handle):
    """Thin RAII wrapper over a gh_qual_handle: exact edge-crossing counts under the engine's float32 test and edge-length
    statistics of one layout (include/graphem_hip.h "layout quality"), and the exact neighbour ranks on the simple graph of
    the same edge list ("embedding quality"), and the hop profile on that graph ("distance preservation").  edges: (E, 2)
    int32, ids kept as given.
    device_id < 0 is the library's host path, which touches no device and returns the same integers."""
    _destroy, _last_error = "gh_qual_destroy", "gh_qual_last_error"

    def __init__(self, edges, n, device_id=0):
        self.device_id = int(device_id)
        edges = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 2)
        self.n, self.E = int(n), int(edges.shape[0])
        self.D = 0   # of the snapshot; 0: no positions yet
        self._create("gh_qual_create", self.device_id, self.n, self.E, ptr(edges))

    def set_positions(self, pos, D=None, ld=None):
        """Snapshot of host float32 positions (gh_qual_set_positions): an (n, D) array, or with D and ld given the first D
        columns of a buffer of n rows of ld floats."""
        pos = np.ascontiguousarray(pos, dtype=np.float32)
        if D is None:
            if pos.ndim != 2 or pos.shape[0] != self.n:
                raise ValueError(f"positions must be ({self.n}, D), got {pos.shape}")
            D = ld = pos.shape[1]
        elif pos.size < self.n * int(ld):
            raise ValueError(f"a buffer of {pos.size} floats is smaller than n * ld = {self.n * int(ld)}")
        self._raise(self.lib.gh_qual_set_positions(self.handle, ptr(pos), int(D), int(ld), 0))
        self.D = int(D)

    def set_positions_device(self, dev_ptr, D, ld=None):
        """Snapshot of (n, D) float32 rows at a device pointer on the handle's device, row stride ld floats (default D)."""
        self._raise(self.lib.gh_qual_set_positions(self.handle, ctypes.c_void_p(int(dev_ptr)), int(D),
                                                   int(D if ld is None else ld), 1))
        self.D = int(D)

    def crossings(self, rows=None):
        """(counts int32, their int sum) for the edge ids `rows`, any order, repeats allowed; None = all edges in order."""
        if rows is not None:
            rows = np.ascontiguousarray(rows, dtype=np.int32).ravel()
            if len(rows) == 0:
                rows = np.zeros(1, dtype=np.int32)[:0]   # (a NULL pointer would mean all edges)
        counts = np.zeros(self.E if rows is None else len(rows), dtype=np.int32)
        total = ctypes.c_int64()
        self._raise(self.lib.gh_qual_crossings(self.handle, len(counts), ptr(rows), ptr(counts), ctypes.byref(total)))
        return counts, int(total.value)

    def pairs(self, pairs):
        """bool per pair of edge ids: do the two edges cross (gh_qual_pairs)."""
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        cross = np.zeros(len(pairs), dtype=np.uint8)
        self._raise(self.lib.gh_qual_pairs(self.handle, len(pairs), ptr(pairs), ptr(cross)))
        return cross.astype(bool)

    def edge_lengths(self):
        """float64 (min, max, sum, sum of squares) of the edge lengths (gh_qual_edge_lengths)."""
        out = np.zeros(4, dtype=np.float64)
        self._raise(self.lib.gh_qual_edge_lengths(self.handle, ptr(out)))
        return out

    def neighbor_ranks(self, rows=None):
        """(indptr int64, neighbors int32, dist2 float32, below int32, equal int32) in CSR form over the source vertex ids
        `rows`, any order, repeats allowed; None = all vertices in order (gh_qual_neighbor_sizes, gh_qual_neighbor_ranks)."""
        if rows is not None:
            rows = np.ascontiguousarray(rows, dtype=np.int32).ravel()
            if len(rows) == 0:
                rows = np.zeros(1, dtype=np.int32)[:0]   # (a NULL pointer would mean all vertices)
        n_rows = self.n if rows is None else len(rows)
        indptr = np.zeros(n_rows + 1, dtype=np.int64)
        self._raise(self.lib.gh_qual_neighbor_sizes(self.handle, n_rows, ptr(rows), ptr(indptr)))
        slots = int(indptr[-1])
        neighbors, dist2 = np.zeros(slots, dtype=np.int32), np.zeros(slots, dtype=np.float32)
        below, equal = np.zeros(slots, dtype=np.int32), np.zeros(slots, dtype=np.int32)
        self._raise(self.lib.gh_qual_neighbor_ranks(self.handle, n_rows, ptr(rows), ptr(neighbors), ptr(dist2), ptr(below), ptr(equal)))
        return indptr, neighbors, dist2, below, equal

    def hop_profile(self, sources=None):
        """The sums of include/graphem_hip.h "distance preservation" over the source vertex ids `sources`, any order, repeats
        allowed; None = all vertices in order (gh_qual_hop_profile).  dict: per hop h = 1 .. H, at entry h - 1, pairs (int64),
        sum_d, sum_d2 (float64), min_d2, max_d2 (float32); per source reach (int64), eccentricity (int32), sum_d_over_h and
        sum_d2_over_h2 (float64)."""
        if sources is not None:
            sources = np.ascontiguousarray(sources, dtype=np.int32).ravel()
            if len(sources) == 0:
                sources = np.zeros(1, dtype=np.int32)[:0]   # (a NULL pointer would mean all vertices)
        S = self.n if sources is None else len(sources)
        cap = max(self.n, 1)   # H <= n - 1
        hop = {"pairs": np.zeros(cap, dtype=np.int64), "sum_d": np.zeros(cap, dtype=np.float64), "sum_d2": np.zeros(cap, dtype=np.float64),
               "min_d2": np.zeros(cap, dtype=np.float32), "max_d2": np.zeros(cap, dtype=np.float32)}
        out = {"reach": np.zeros(S, dtype=np.int64), "eccentricity": np.zeros(S, dtype=np.int32),
               "sum_d_over_h": np.zeros(S, dtype=np.float64), "sum_d2_over_h2": np.zeros(S, dtype=np.float64)}
        H = ctypes.c_int64()
        self._raise(self.lib.gh_qual_hop_profile(self.handle, S, ptr(sources), cap, ctypes.byref(H), *(ptr(a) for a in hop.values()),
                                                 *(ptr(a) for a in out.values())))
        return {**{key: a[:H.value].copy() for key, a in hop.items()}, **out}

    def _centres(self, centres):
        centres = np.array(centres, dtype=np.float32, order="C")   # a copy: gh_qual_kmeans writes it
        if centres.ndim != 2 or centres.shape[0] < 1:
            raise ValueError(f"centres must be (k, D) with k >= 1, got {centres.shape}")
        if self.D and centres.shape[1] != self.D:
            raise ValueError(f"centres of dimension {centres.shape[1]} for positions of dimension {self.D}")
        return centres

    def position_rows(self, rows):
        """float32 (len(rows), D): the snapshot's rows at the vertex ids `rows` (gh_qual_position_rows)."""
        rows = np.ascontiguousarray(rows, dtype=np.int32).ravel()
        out = np.zeros((len(rows), self.D), dtype=np.float32)
        if len(rows):
            self._raise(self.lib.gh_qual_position_rows(self.handle, len(rows), ptr(rows), ptr(out)))
        return out

    def kmeans_assign(self, centres):
        """(labels int32, d2 float32) of every vertex under the (k, D) centres: the least nearest centre and the float32
        squared distance to it (include/graphem_hip.h "embedding clusters", gh_qual_kmeans_assign)."""
        centres = self._centres(centres)
        labels, d2 = np.zeros(self.n, dtype=np.int32), np.zeros(self.n, dtype=np.float32)
        self._raise(self.lib.gh_qual_kmeans_assign(self.handle, len(centres), ptr(centres), ptr(labels), ptr(d2)))
        return labels, d2

    def kmeans(self, centres, max_iter=300):
        """The Lloyd loop from the (k, D) start centres with exact centre updates (gh_qual_kmeans).  dict: labels (int32),
        centers (float32 (k, D)), d2 (float32), counts (int64), n_iter (the number of updates) and converged."""
        centres = self._centres(centres)
        k = len(centres)
        labels, d2 = np.zeros(self.n, dtype=np.int32), np.zeros(self.n, dtype=np.float32)
        counts = np.zeros(k, dtype=np.int64)
        n_iter, converged = ctypes.c_int32(), ctypes.c_int32()
        self._raise(self.lib.gh_qual_kmeans(self.handle, k, ptr(centres), int(max_iter), ptr(labels), ptr(d2), ptr(counts),
                                            ctypes.byref(n_iter), ctypes.byref(converged)))
        return {"labels": labels, "centers": centres, "d2": d2, "counts": counts, "n_iter": int(n_iter.value),
                "converged": bool(converged.value)}

    def kmeans_seed_step(self, vertex, first):
        """float32 (n,): the handle's running minimum of d2(x_w, x_vertex) over the steps since the last one with `first`
        set (gh_qual_kmeans_seed_step)."""
        min_d2 = np.zeros(self.n, dtype=np.float32)
        self._raise(self.lib.gh_qual_kmeans_seed_step(self.handle, int(vertex), int(bool(first)), ptr(min_d2)))
        return min_d2

    def cluster_distance_sums(self, labels, k, rows=None):
        """float64 (len(rows), k): per row vertex and cluster the sum of the distances to the cluster's other members
        (gh_qual_cluster_distance_sums).  labels: n ids in [0, k); rows: vertex ids, any order, repeats allowed; None = all
        vertices in order."""
        labels = np.ascontiguousarray(labels, dtype=np.int32).ravel()
        if len(labels) != self.n:
            raise ValueError(f"{len(labels)} labels for {self.n} vertices")
        if rows is not None:
            rows = np.ascontiguousarray(rows, dtype=np.int32).ravel()
            if len(rows) == 0:
                rows = np.zeros(1, dtype=np.int32)[:0]   # (a NULL pointer would mean all vertices)
        n_rows = self.n if rows is None else len(rows)
        sums = np.zeros((n_rows, max(int(k), 0)), dtype=np.float64)
        self._raise(self.lib.gh_qual_cluster_distance_sums(self.handle, int(k), ptr(labels), n_rows, ptr(rows), ptr(sums)))
        return sums

    def knn_vote(self, k, train, train_labels=None, rows=None, neighbors=True, d2=True, pred=True, votes=True):
        """(neighbors (R, k) int32, d2 (R, k) float32, pred (R,) int32, votes (R,) int32): the k nearest training vertices
        of every query row under (d2, vertex id), unused slots -1 and +inf, and the vote of their classes
        (include/graphem_hip.h "node classification", gh_qual_knn_vote).  train: distinct vertex ids; train_labels: their
        classes, >= 0, or None (then pred and votes are None); rows: vertex ids, any order, repeats allowed; None = all
        vertices in order.  A part not asked for is None."""
        k = int(k)
        train = np.ascontiguousarray(train, dtype=np.int32).ravel()
        if train_labels is not None:
            train_labels = np.ascontiguousarray(train_labels, dtype=np.int32).ravel()
            if len(train_labels) != len(train):
                raise ValueError(f"{len(train_labels)} labels for {len(train)} training vertices")
            if len(train) == 0:
                train_labels = np.zeros(1, dtype=np.int32)[:0]   # (a NULL pointer would mean no labels)
        if rows is not None:
            rows = np.ascontiguousarray(rows, dtype=np.int32).ravel()
            if len(rows) == 0:
                rows = np.zeros(1, dtype=np.int32)[:0]   # (a NULL pointer would mean all vertices)
        n_rows = self.n if rows is None else len(rows)
        slots = (n_rows, max(k, 0))
        out_i = np.zeros(slots, dtype=np.int32) if neighbors else None
        out_d = np.zeros(slots, dtype=np.float32) if d2 else None
        out_p = np.zeros(n_rows, dtype=np.int32) if pred and train_labels is not None else None
        out_v = np.zeros(n_rows, dtype=np.int32) if votes and train_labels is not None else None
        self._raise(self.lib.gh_qual_knn_vote(self.handle, k, len(train), ptr(train), ptr(train_labels), n_rows, ptr(rows),
                                              ptr(out_i), ptr(out_d), ptr(out_p), ptr(out_v)))
        return out_i, out_d, out_p, out_v


class EdgeListParser(BudgetHandle):
    """Thin RAII wrapper over a gh_ingest_handle: the text of an edge list to (vertices, edges) under the rule of
    include/graphem_hip.h "edge-list ingestion".  device_id < 0 is the library's host path, which touches no device and
    returns the same arrays bit for bit.  Memory budget: device bytes of working state per chunk of text, 4 GiB by default,
    at least MIN_BUDGET.  A handle can parse again; each parse replaces its result."""
    _destroy, _last_error, _set_budget = "gh_ingest_destroy", "gh_ingest_last_error", "gh_ingest_set_memory_budget"
    FORMATS = {"snap": 0, "edges": 1, "mtx": 2}
    VERTICES_FROM = {"edges": 0, "rows": 1}
    MIN_BUDGET = 4096

    def __init__(self, device_id=0):
        self.device_id = int(device_id)
        self.rows = self.n_edges = self.n_vertices = 0
        self._create("gh_ingest_create", self.device_id)

    def _codes(self, fmt, vertices_from):
        if fmt not in self.FORMATS:
            raise ValueError(f"format must be one of {sorted(self.FORMATS)}, got {fmt!r}")
        if vertices_from not in self.VERTICES_FROM:
            raise ValueError(f"vertices_from must be 'edges' or 'rows', got {vertices_from!r}")
        return self.FORMATS[fmt], self.VERTICES_FROM[vertices_from]

    def _counts(self):
        r, e, v = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        self._raise(self.lib.gh_ingest_counts(self.handle, ctypes.byref(r), ctypes.byref(e), ctypes.byref(v)))
        self.rows, self.n_edges, self.n_vertices = int(r.value), int(e.value), int(v.value)

    def parse(self, data, fmt="snap", directed=False, vertices_from="edges"):
        """Parses the bytes of a file (bytes, bytearray or a uint8 array); a malformed line is a ValueError naming it."""
        f, vf = self._codes(fmt, vertices_from)
        buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
        self._raise(self.lib.gh_ingest_parse(self.handle, ptr(buf) if buf.size else None, int(buf.size), f, int(bool(directed)), vf))
        self._counts()

    def parse_uploaded(self, data, dev_ptr, fmt="snap", directed=False, vertices_from="edges"):
        """parse() for a text whose bytes are also on the handle's device already, 16-byte aligned at dev_ptr."""
        f, vf = self._codes(fmt, vertices_from)
        buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
        self._raise(self.lib.gh_ingest_parse_uploaded(self.handle, ptr(buf) if buf.size else None, ctypes.c_void_p(int(dev_ptr)),
                                                      int(buf.size), f, int(bool(directed)), vf))
        self._counts()

    def chunking(self):
        """(bytes of text per chunk under the current budget, chunks the last parse took -- 0 on the host path)."""
        cb, ch = ctypes.c_int64(), ctypes.c_int64()
        self._raise(self.lib.gh_ingest_chunking(self.handle, ctypes.byref(cb), ctypes.byref(ch)))
        return int(cb.value), int(ch.value)

    def vertices(self):
        """int64 (n_vertices,): the sorted distinct labels."""
        out = np.zeros(self.n_vertices, dtype=np.int64)
        self._raise(self.lib.gh_ingest_copy_vertices(self.handle, ptr(out)))
        return out

    def edges(self, relabel=False):
        """int64 (n_edges, 2): labels, or with relabel their ranks in vertices()."""
        out = np.zeros((self.n_edges, 2), dtype=np.int64)
        self._raise(self.lib.gh_ingest_copy_edges(self.handle, int(bool(relabel)), ptr(out)))
        return out
