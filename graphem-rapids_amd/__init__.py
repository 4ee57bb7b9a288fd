"""graphem_rapids_amd: MI355X-native force-directed graph embedding.

Drop-in for one path of sashakolpakov/graphem-rapids: create_graphem() /
run_layout() / get_positions() (reference graphem_rapids/__init__.py:78-136), backed by
hand-written HIP kernels for gfx950 behind the C ABI in include/graphem_hip.h.
"""
from .backend_selection import BackendConfig, check_hip_availability, get_optimal_backend, estimate_memory_usage
from .embedder_hip import GraphEmbedderHIP
from .memory_management import (MemoryManager, cleanup_gpu_memory, get_gpu_memory_info, get_optimal_chunk_size,
                                monitor_memory_usage)
from .generators import (erdos_renyi_graph, generate_random_regular, erdos_renyi_edges, random_regular_edges, planted_partition_edges,
                         edges_to_adjacency, load_snap_edge_list,
                         generate_sbm, generate_ba, generate_ws, generate_power_cluster, generate_scale_free,
                         generate_geometric, generate_road_network, generate_bipartite_graph, generate_balanced_tree,
                         generate_caveman, generate_relaxed_caveman, sbm_edges, bipartite_edges, geometric_edges,
                         barabasi_albert_edges, caveman_edges, road_network_edges, balanced_tree_edges,
                         watts_strogatz_edges, powerlaw_cluster_edges, scale_free_edges, relaxed_caveman_edges)
from .influence import (InfluenceGraph, influence_spread, ndlib_estimated_influence, greedy_seed_selection,
                        run_influence_benchmark, RRCollection, max_coverage, ris_seed_selection, kshell_seed_selection,
                        arc_probabilities, trivalency_probabilities, lt_weights, linear_threshold)
from .centrality import (CentralityGraph, betweenness_centrality, load_centrality, closeness_centrality, pagerank,
                         eigenvector_centrality_numpy, run_benchmark, benchmark_correlations)
from . import graphstats
from .graphstats import (connected_components, number_connected_components, is_connected, largest_connected_component,
                         eccentricity, diameter, radius, average_shortest_path_length, triangles, clustering,
                         average_clustering, transitivity, graph_summary, print_graph_summary)
from . import communities
from .communities import (modularity, louvain_communities, louvain_partitions, community_labels, adjusted_rand_index,
                          normalized_mutual_info)
from . import cores
from .cores import (core_number, onion_layers, degeneracy, k_core, k_shell, k_crust, k_corona, truss_number, k_truss)
from . import links
from .links import (link_scores, jaccard_coefficient, adamic_adar_index, resource_allocation_index, preferential_attachment,
                    link_candidates, top_links, split_edges, embedding_link_scores, ranking_auc, average_precision,
                    link_prediction_benchmark)
from . import quality
from .quality import (edge_crossing_counts, edge_crossings, estimate_edge_crossings, edge_length_stats, layout_quality,
                      neighbor_ranks, link_auc, neighborhood_preservation, embedding_quality,
                      hop_profile, layout_stress, hop_distance_correlation, distance_quality)
from . import clusters
from .clusters import (kmeans, kmeans_plusplus, nearest_center, silhouette_samples, silhouette_score, cluster_recovery)
from . import classify
from .classify import (knn_neighbors, knn_classify, label_propagation, split_labels, accuracy, confusion_matrix, macro_f1,
                       node_classification_benchmark, CLASSIFY_METHODS)
from . import datasets
from .datasets import (read_edge_list, parse_edge_list, load_dataset, load_dataset_as_networkx, load_dataset_adjacency,
                       list_available_datasets, get_data_directory, SNAPDataset, NetworkRepositoryDataset,
                       SemanticScholarDataset)
from .visualization import (spearman_matrix, bootstrap_spearman, report_corr, report_full_correlation_matrix,
                            plot_radial_vs_centrality, display_benchmark_results)

__version__ = "0.1.0"


def create_graphem(adjacency, n_components=2, backend=None, **kwargs):
    """Same factory signature as the reference (graphem_rapids/__init__.py:78-136).
    backend: None / 'auto' / 'hip' -> GraphEmbedderHIP; anything else raises ValueError."""
    config = BackendConfig(n_vertices=adjacency.shape[0], n_components=n_components)
    config.force_backend = backend
    get_optimal_backend(config)  # validates the name
    return GraphEmbedderHIP(adjacency, n_components, **kwargs)


def get_backend_info():
    """Availability report, shaped like the reference's get_backend_info (__init__.py:139-169)."""
    hip = check_hip_availability()
    return {
        "hip_library": hip["library"],
        "hip_version": hip["version"],
        "cuda_available": hip["device_count"] > 0,
        "cuda_device_count": hip["device_count"],
        "recommended_backend": "hip" if hip["library"] and hip["device_count"] > 0 else None,
    }


def graphem_seed_selection(embedder, k, num_iterations=20):
    """Caller contract of the reference's influence.graphem_seed_selection (influence.py:10-37):
    run the layout, pick the k vertices farthest from the origin."""
    import numpy as np
    embedder.run_layout(num_iterations=num_iterations)
    engine = getattr(embedder, "_engine", None)
    if engine is not None and 1 <= k <= min(64, embedder.n):
        # radial norm + top-k on the device, k ids come back instead of (n, D) positions
        return engine.radial_topk(k).tolist()
    radial = np.linalg.norm(np.array(embedder.positions), axis=1)
    return np.argsort(-radial)[:k].tolist()


__all__ = ["create_graphem", "get_backend_info", "GraphEmbedderHIP", "BackendConfig", "get_optimal_backend",
           "check_hip_availability", "estimate_memory_usage", "erdos_renyi_graph", "generate_random_regular",
           "erdos_renyi_edges", "random_regular_edges", "planted_partition_edges", "edges_to_adjacency", "load_snap_edge_list",
           "graphem_seed_selection", "MemoryManager", "cleanup_gpu_memory", "get_gpu_memory_info",
           "get_optimal_chunk_size", "monitor_memory_usage", "InfluenceGraph", "influence_spread",
           "ndlib_estimated_influence", "greedy_seed_selection", "run_influence_benchmark", "RRCollection", "max_coverage",
           "ris_seed_selection", "kshell_seed_selection", "arc_probabilities", "trivalency_probabilities",
           "lt_weights", "linear_threshold",
           "CentralityGraph", "betweenness_centrality", "load_centrality", "closeness_centrality", "pagerank",
           "eigenvector_centrality_numpy", "run_benchmark", "benchmark_correlations",
           "generate_sbm", "generate_ba", "generate_ws", "generate_power_cluster", "generate_scale_free",
           "generate_geometric", "generate_road_network", "generate_bipartite_graph", "generate_balanced_tree",
           "generate_caveman", "generate_relaxed_caveman", "sbm_edges", "bipartite_edges", "geometric_edges",
           "barabasi_albert_edges", "caveman_edges", "road_network_edges", "balanced_tree_edges",
           "watts_strogatz_edges", "powerlaw_cluster_edges", "scale_free_edges", "relaxed_caveman_edges",
           "graphstats", "connected_components", "number_connected_components", "is_connected",
           "largest_connected_component", "eccentricity", "diameter", "radius", "average_shortest_path_length",
           "triangles", "clustering", "average_clustering", "transitivity", "graph_summary", "print_graph_summary",
           "spearman_matrix", "bootstrap_spearman", "report_corr", "report_full_correlation_matrix",
           "plot_radial_vs_centrality", "display_benchmark_results",
           "communities", "modularity", "louvain_communities", "louvain_partitions", "community_labels",
           "adjusted_rand_index", "normalized_mutual_info",
           "cores", "core_number", "onion_layers", "degeneracy", "k_core", "k_shell", "k_crust", "k_corona", "truss_number",
           "k_truss",
           "links", "link_scores", "jaccard_coefficient", "adamic_adar_index", "resource_allocation_index",
           "preferential_attachment", "link_candidates", "top_links", "split_edges", "embedding_link_scores", "ranking_auc",
           "average_precision", "link_prediction_benchmark",
           "quality", "edge_crossing_counts", "edge_crossings", "estimate_edge_crossings", "edge_length_stats",
           "layout_quality", "neighbor_ranks", "link_auc", "neighborhood_preservation", "embedding_quality",
           "hop_profile", "layout_stress", "hop_distance_correlation", "distance_quality",
           "clusters", "kmeans", "kmeans_plusplus", "nearest_center", "silhouette_samples", "silhouette_score",
           "cluster_recovery",
           "classify", "knn_neighbors", "knn_classify", "label_propagation", "split_labels", "accuracy", "confusion_matrix",
           "macro_f1", "node_classification_benchmark", "CLASSIFY_METHODS",
           "datasets", "read_edge_list", "parse_edge_list", "load_dataset", "load_dataset_as_networkx",
           "load_dataset_adjacency", "list_available_datasets", "get_data_directory", "SNAPDataset",
           "NetworkRepositoryDataset", "SemanticScholarDataset"]
