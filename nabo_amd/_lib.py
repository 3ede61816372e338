"""ctypes binding of libnabo_knn.so (include/nabo_knn.h).  No torch, no CPU fallback:
if the HIP library is missing or no GPU is visible, every compute entry point raises."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# NABO_KNN_SO: load another build of the library (a parent / branch A/B; _build.build(out=...)) WITHOUT overwriting the product's
SO_PATH = os.environ.get("NABO_KNN_SO") or os.path.join(HERE, "libnabo_knn.so")

EUCLIDEAN = 0
MOD_CANBERRA = 1
COSINE = 2          # extension: not in the reference (include/nabo_knn.h)
MAX_COMPS = 128
MAX_K = 56

E_INVALID, E_NODEVICE, E_HIP, E_NOMEM, E_UNSUPPORTED, E_COMM = -1, -2, -3, -4, -5, -6

_lib = None

# every symbol include/nabo_knn.h declares (tests check the .so exports exactly these)
SYMBOLS = [
    "nabo_version", "nabo_last_error", "nabo_device_count", "nabo_knn", "nabo_pairwise",
    "nabo_index_create", "nabo_index_destroy", "nabo_index_set_option", "nabo_query_plan", "nabo_index_set_ref", "nabo_index_set_mask", "nabo_index_query", "nabo_index_query_async", "nabo_index_query_wait",
    "nabo_index_query_candidates",
    "nabo_index_last_stats", "nabo_index_last_kernel", "nabo_index_last_passes", "nabo_index_last_row_pass", "nabo_merge_topk", "nabo_snn_counts", "nabo_pyset_order", "nabo_component_labels", "nabo_group_edges", "nabo_score_null", "nabo_score_null_edges", "nabo_dev_malloc", "nabo_dev_free",
    "nabo_memcpy_h2d", "nabo_memcpy_d2h", "nabo_dev_synchronize", "nabo_dev_mem_info",
    "nabo_comm_unique_id", "nabo_comm_create", "nabo_comm_create_all", "nabo_comm_create_loopback", "nabo_comm_destroy",
    "nabo_comm_rank", "nabo_comm_world", "nabo_comm_transport_ranks", "nabo_comm_abort", "nabo_comm_set_timeout", "nabo_comm_set_ref_shards", "nabo_comm_barrier", "nabo_comm_allreduce_max_f64", "nabo_candidates_per_shard",
    "nabo_sharded_query", "nabo_sharded_last_stats", "nabo_knn_devices",
]

# every symbol include/nabo_graph.h declares (hop distances on the reference graph; kept apart from SYMBOLS, which
# pins include/nabo_knn.h)
GRAPH_SYMBOLS = ["nabo_refgraph_create", "nabo_refgraph_destroy", "nabo_refgraph_set_option", "nabo_refgraph_group_hops",
                 "nabo_refgraph_last_stats", "nabo_refgraph_last_local_nodes"]


# every symbol include/nabo_cluster.h declares (classification of target nodes, levels around node sets)
CLUSTER_SYMBOLS = ["nabo_classify_targets", "nabo_refgraph_set_levels", "nabo_cluster_last_device_ms"]

# every symbol include/nabo_de.h declares (the Mann-Whitney differential-expression test)
DE_SYMBOLS = ["nabo_de_test", "nabo_de_last_device_ms"]

# every symbol include/nabo_pca.h declares (PCA projection of sparse cells, per-gene statistics)
PCA_SYMBOLS = ["nabo_pca_project", "nabo_gene_stats", "nabo_pca_last_device_ms"]

# every symbol include/nabo_pca_fit.h declares (mean and covariance of the scaled cells: the exact PCA fit)
PCA_FIT_SYMBOLS = ["nabo_pca_cov", "nabo_pca_cov_last_phase_ms"]

# every symbol include/nabo_qc.h declares (per-cell quality-control sums)
QC_SYMBOLS = ["nabo_cell_qc", "nabo_qc_last_device_ms"]

# every symbol include/nabo_layout.h declares (ForceAtlas2 layout of the reference graph, exact repulsion)
LAYOUT_SYMBOLS = ["nabo_layout_create", "nabo_layout_destroy", "nabo_layout_set_params", "nabo_layout_set_state",
                  "nabo_layout_get_state", "nabo_layout_run", "nabo_layout_last_forces", "nabo_layout_last_ms",
                  "nabo_layout_geometry"]

# every symbol include/nabo_umap.h declares (UMAP embedding: fuzzy k-NN graph, synchronous epochs)
UMAP_SYMBOLS = ["nabo_umap_create", "nabo_umap_destroy", "nabo_umap_set_params", "nabo_umap_set_knn", "nabo_umap_fit_knn", "nabo_umap_set_graph",
                "nabo_umap_graph_size", "nabo_umap_get_graph", "nabo_umap_set_embedding", "nabo_umap_get_embedding",
                "nabo_umap_run", "nabo_umap_rewind", "nabo_umap_last_epoch_counts", "nabo_umap_last_ms", "nabo_umap_geometry"]

# every symbol include/nabo_umap_transform.h declares (UMAP transform: target cells placed in a fitted reference embedding)
UMAP_TRANSFORM_SYMBOLS = ["nabo_umap_transform_create", "nabo_umap_transform_destroy", "nabo_umap_transform_set_params",
                          "nabo_umap_transform_set_embedding", "nabo_umap_transform_set_cells", "nabo_umap_transform_query",
                          "nabo_umap_transform_set_knn", "nabo_umap_transform_set_graph", "nabo_umap_transform_get_graph",
                          "nabo_umap_transform_set_positions", "nabo_umap_transform_get_positions", "nabo_umap_transform_run",
                          "nabo_umap_transform_rewind", "nabo_umap_transform_last_run_counts", "nabo_umap_transform_last_ms",
                          "nabo_umap_transform_geometry"]

# every symbol include/nabo_community.h declares (communities of the reference graph: seeded synchronous Louvain)
COMMUNITY_SYMBOLS = ["nabo_community_create", "nabo_community_destroy", "nabo_community_set_params", "nabo_community_run",
                     "nabo_community_labels", "nabo_community_history", "nabo_community_modularity", "nabo_community_split",
                     "nabo_community_level_size", "nabo_community_get_level", "nabo_community_set_comm", "nabo_community_get_comm",
                     "nabo_community_sweep", "nabo_community_aggregate", "nabo_community_rewind", "nabo_community_last_ms",
                     "nabo_community_geometry"]

# every symbol include/nabo_agglom.h declares (greedy modularity agglomeration on the handle of nabo_community.h)
AGGLOM_SYMBOLS = ["nabo_community_agglomerate", "nabo_community_dendrogram", "nabo_community_agglom_info", "nabo_community_cut",
                  "nabo_community_match_pass", "nabo_community_match", "nabo_community_agglom_ms"]

# every symbol include/nabo_potential.h declares (differentiation potential: a sparse solve by Jacobi PCG)
POTENTIAL_SYMBOLS = ["nabo_potential_create", "nabo_potential_destroy", "nabo_potential_set_params", "nabo_potential_graph_size",
                     "nabo_potential_prepare", "nabo_potential_get_prepared", "nabo_potential_iterate", "nabo_potential_get_state",
                     "nabo_potential_set_state", "nabo_potential_finish", "nabo_potential_solve", "nabo_potential_info",
                     "nabo_potential_last_ms", "nabo_potential_geometry"]

# every symbol include/nabo_bundle.h declares (edge bundling: density-guided advection of the laid-out graph's edges)
BUNDLE_SYMBOLS = ["nabo_bundle_create", "nabo_bundle_destroy", "nabo_bundle_set_params", "nabo_bundle_set_option",
                  "nabo_bundle_get_points", "nabo_bundle_set_points", "nabo_bundle_resample", "nabo_bundle_density",
                  "nabo_bundle_field", "nabo_bundle_advect", "nabo_bundle_smooth", "nabo_bundle_run", "nabo_bundle_result",
                  "nabo_bundle_last_ms", "nabo_bundle_geometry", "nabo_bundle_blur_weights"]

# every symbol include/nabo_render.h declares (the rasteriser: nodes and edges to integer images and an RGBA picture)
RENDER_SYMBOLS = ["nabo_render_create", "nabo_render_destroy", "nabo_render_clear", "nabo_render_set_option",
                  "nabo_render_add_polylines", "nabo_render_add_edges", "nabo_render_add_bundle", "nabo_render_add_nodes",
                  "nabo_render_edge_counts", "nabo_render_node_counts", "nabo_render_node_sums", "nabo_render_compose",
                  "nabo_render_last_ms", "nabo_render_alpha_lut", "nabo_render_geometry"]

# every symbol include/nabo_ingest.h declares (Matrix Market counts to the cell and gene indexes; CSR to CSC)
INGEST_SYMBOLS = ["nabo_mtx_create", "nabo_mtx_feed", "nabo_mtx_finish", "nabo_mtx_get_csr", "nabo_mtx_get_csc", "nabo_mtx_free",
                  "nabo_mtx_geometry", "nabo_mtx_last_device_ms", "nabo_csr_transpose"]

# every symbol include/nabo_counts.h declares (the Matrix Market writer; the remap behind subsetting and merging counts)
COUNTS_SYMBOLS = ["nabo_mtxw_create", "nabo_mtxw_read", "nabo_mtxw_last_device_ms", "nabo_mtxw_free", "nabo_mtxw_geometry",
                  "nabo_counts_remap"]

# every symbol include/nabo_csv.h declares (a dense CSV table of numbers to its entries by row and by column)
CSV_SYMBOLS = ["nabo_csv_create", "nabo_csv_set_first_line", "nabo_csv_feed", "nabo_csv_finish", "nabo_csv_get_rows", "nabo_csv_get_cols",
               "nabo_csv_get_row_names", "nabo_csv_stats", "nabo_csv_last_device_ms", "nabo_csv_geometry", "nabo_csv_free"]

# what include/nabo_knn_inspect.h declares (a look into an index, for tests and tools)
INSPECT_SYMBOLS = ["nabo_index_stream_order"]


class NaboError(RuntimeError):
    pass


def lib():
    """Load libnabo_knn.so; fail loudly if it has not been built (python -m nabo_amd._build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise NaboError("libnabo_knn.so not found at %s -- build it with `python -m nabo_amd._build` "
                        "(there is no CPU fallback)" % SO_PATH)
    L = C.CDLL(SO_PATH)
    vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    L.nabo_version.restype = C.c_char_p
    L.nabo_last_error.restype = C.c_char_p
    L.nabo_device_count.restype = C.c_int
    L.nabo_knn.argtypes = [vp, i64, vp, i64, i32, i32, i32, dbl, vp, i32, vp, vp, i32]
    L.nabo_pairwise.argtypes = [vp, i64, vp, i64, i32, i32, dbl, vp, i32]
    L.nabo_index_create.argtypes = [C.POINTER(vp), i32, i64, i32, i32, dbl, i64]
    L.nabo_index_destroy.argtypes = [vp]
    L.nabo_index_set_option.argtypes = [vp, C.c_char_p, i64]
    L.nabo_query_plan.argtypes = [i64, i32, i32, i64, i32, i32, i32, i32, C.c_char_p, C.c_char_p, C.POINTER(i64), C.c_char_p, C.c_size_t]
    L.nabo_index_set_ref.argtypes = [vp, vp, i32, vp]
    L.nabo_index_set_mask.argtypes = [vp, vp]
    L.nabo_index_query.argtypes = [vp, vp, i32, i64, i32, i32, vp, vp, i32]
    L.nabo_index_query_async.argtypes = [vp, vp, i32, i64, i32, i32, vp, vp, i32]
    L.nabo_index_query_wait.argtypes = [vp]
    L.nabo_index_query_candidates.argtypes = [vp, vp, i32, i64, i32, vp, vp, vp]
    L.nabo_index_last_stats.argtypes = [vp, C.POINTER(dbl), C.POINTER(i64)]
    L.nabo_index_last_kernel.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.nabo_index_last_passes.argtypes = [vp, C.POINTER(i64)]
    L.nabo_index_last_row_pass.argtypes = [vp, vp, i64]
    L.nabo_index_stream_order.argtypes = [vp, vp, C.POINTER(i64), vp, C.POINTER(i64)]
    L.nabo_merge_topk.argtypes = [i32, vp, vp, i32, i64, i32, i32, i32, vp, vp]
    L.nabo_snn_counts.argtypes = [i32, vp, i64, vp, i64, i32, vp]
    L.nabo_dev_malloc.argtypes = [i32, C.POINTER(vp), C.c_size_t]
    L.nabo_dev_free.argtypes = [i32, vp]
    L.nabo_memcpy_h2d.argtypes = [i32, vp, vp, C.c_size_t]
    L.nabo_memcpy_d2h.argtypes = [i32, vp, vp, C.c_size_t]
    L.nabo_dev_synchronize.argtypes = [i32]
    L.nabo_dev_mem_info.argtypes = [i32, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.nabo_comm_unique_id.argtypes = [vp]
    L.nabo_comm_create.argtypes = [C.POINTER(vp), i32, i32, i32, vp]
    L.nabo_comm_create_all.argtypes = [C.POINTER(vp), C.POINTER(i32), i32]
    L.nabo_comm_create_loopback.argtypes = [C.POINTER(vp), C.POINTER(i32), i32]
    L.nabo_comm_destroy.argtypes = [vp]
    L.nabo_comm_rank.argtypes = [vp]
    L.nabo_comm_world.argtypes = [vp]
    L.nabo_comm_transport_ranks.argtypes = [vp]
    L.nabo_comm_set_ref_shards.argtypes = [vp, i32]
    L.nabo_comm_abort.argtypes = [vp]
    L.nabo_comm_set_timeout.argtypes = [vp, dbl]
    L.nabo_comm_barrier.argtypes = [vp]
    L.nabo_comm_allreduce_max_f64.argtypes = [vp, C.POINTER(dbl)]
    L.nabo_candidates_per_shard.argtypes = [i32, i32, i64]
    L.nabo_sharded_query.argtypes = [vp, vp, vp, i64, i32, i32, vp, vp, i32]
    L.nabo_sharded_last_stats.argtypes = [vp, C.POINTER(dbl), C.POINTER(i64)]
    L.nabo_knn_devices.argtypes = [vp, i64, vp, i64, i32, i32, i32, dbl, vp, i32, C.POINTER(i32), i32, i32, vp, vp]
    L.nabo_refgraph_create.argtypes = [C.POINTER(vp), i32, i64, vp, vp]
    L.nabo_refgraph_destroy.argtypes = [vp]
    L.nabo_refgraph_set_option.argtypes = [vp, C.c_char_p, i64]
    L.nabo_refgraph_group_hops.argtypes = [vp, i64, vp, vp, vp, vp, vp]
    L.nabo_refgraph_last_stats.argtypes = [vp, C.POINTER(dbl), C.POINTER(i64)]
    L.nabo_refgraph_last_local_nodes.argtypes = [vp, i64, vp]
    L.nabo_classify_targets.argtypes = [i32, i64, vp, i32, i64, vp, vp, vp, dbl, i64, dbl, vp, vp, vp, vp]
    L.nabo_refgraph_set_levels.argtypes = [vp, i64, vp, vp, i32, vp]
    L.nabo_cluster_last_device_ms.argtypes = [C.POINTER(dbl)]
    L.nabo_de_test.argtypes = [i32, i64, i64, vp, vp, vp, vp, i64, vp, vp, vp, vp, i64, vp, vp, i64, vp, vp, dbl, dbl, i64] + [vp] * 10
    L.nabo_de_last_device_ms.argtypes = [C.POINTER(dbl), C.POINTER(i64)]
    L.nabo_pca_project.argtypes = [i32, i64, i64, vp, vp, vp, vp, vp, i64, vp, vp, vp, i32, vp, i64, vp, i64, vp]
    L.nabo_gene_stats.argtypes = [i32, i64, i64, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp]
    L.nabo_pca_last_device_ms.argtypes = [C.POINTER(dbl), C.POINTER(i64)]
    L.nabo_pca_cov.argtypes = [i32, i64, i64, vp, vp, vp, vp, vp, i64, vp, vp, i64, vp, i64, vp, vp]
    L.nabo_pca_cov_last_phase_ms.argtypes = [C.POINTER(dbl)]
    L.nabo_cell_qc.argtypes = [i32, i64, i64, vp, vp, vp, i32, vp, i64, vp, i64, vp, vp]
    L.nabo_qc_last_device_ms.argtypes = [C.POINTER(dbl), C.POINTER(i64)]
    L.nabo_layout_create.argtypes = [C.POINTER(vp), i32, i64, vp, vp, vp]
    L.nabo_layout_destroy.argtypes = [vp]
    L.nabo_layout_set_params.argtypes = [vp, i32, dbl, dbl, dbl, i32, dbl, dbl]
    L.nabo_layout_set_state.argtypes = [vp, vp, vp, vp, vp, dbl, dbl]
    L.nabo_layout_get_state.argtypes = [vp, vp, vp, vp, vp, C.POINTER(dbl), C.POINTER(dbl)]
    L.nabo_layout_run.argtypes = [vp, i64, C.POINTER(i64)]
    L.nabo_layout_last_forces.argtypes = [vp, vp, vp, vp, C.POINTER(dbl)]
    L.nabo_layout_last_ms.argtypes = [vp, C.POINTER(dbl), C.POINTER(i64)]
    L.nabo_layout_geometry.argtypes = [i64, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.nabo_umap_create.argtypes = [C.POINTER(vp), i32, i64, i32]
    L.nabo_umap_destroy.argtypes = [vp]
    L.nabo_umap_set_params.argtypes = [vp, i64, i32, dbl, dbl, dbl, C.c_uint64]
    L.nabo_umap_set_knn.argtypes = [vp, vp, vp, i32]
    L.nabo_umap_fit_knn.argtypes = [vp, vp, i32, i32, i32, dbl]
    L.nabo_umap_set_graph.argtypes = [vp, vp, vp, vp]
    L.nabo_umap_graph_size.argtypes = [vp, C.POINTER(i64), C.POINTER(dbl)]
    L.nabo_umap_get_graph.argtypes = [vp, vp, vp, vp, vp, vp]
    L.nabo_umap_set_embedding.argtypes = [vp, vp]
    L.nabo_umap_get_embedding.argtypes = [vp, vp]
    L.nabo_umap_run.argtypes = [vp, i64, C.POINTER(i64)]
    L.nabo_umap_rewind.argtypes = [vp]
    L.nabo_umap_last_epoch_counts.argtypes = [vp, vp, vp, vp]
    L.nabo_umap_last_ms.argtypes = [vp, C.POINTER(dbl), C.POINTER(i64)]
    L.nabo_umap_geometry.argtypes = [C.POINTER(i32)]
    L.nabo_umap_transform_create.argtypes = [C.POINTER(vp), i32, i64, i32]
    L.nabo_umap_transform_destroy.argtypes = [vp]
    L.nabo_umap_transform_set_params.argtypes = [vp, i64, i32, dbl, dbl, dbl, C.c_uint64]
    L.nabo_umap_transform_set_embedding.argtypes = [vp, vp]
    L.nabo_umap_transform_set_cells.argtypes = [vp, vp, i32, i32, dbl]
    L.nabo_umap_transform_query.argtypes = [vp, i64, i64, vp, i32]
    L.nabo_umap_transform_set_knn.argtypes = [vp, i64, i64, vp, vp, i32]
    L.nabo_umap_transform_set_graph.argtypes = [vp, i64, i64, vp, vp, i32]
    L.nabo_umap_transform_get_graph.argtypes = [vp, vp, vp, vp]
    L.nabo_umap_transform_set_positions.argtypes = [vp, vp]
    L.nabo_umap_transform_get_positions.argtypes = [vp, vp]
    L.nabo_umap_transform_run.argtypes = [vp, i64, C.POINTER(i64)]
    L.nabo_umap_transform_rewind.argtypes = [vp]
    L.nabo_umap_transform_last_run_counts.argtypes = [vp, vp, vp, vp]
    L.nabo_umap_transform_last_ms.argtypes = [vp, C.POINTER(dbl)]
    L.nabo_umap_transform_geometry.argtypes = [C.POINTER(i32)]
    L.nabo_community_create.argtypes = [C.POINTER(vp), i32, i64, vp, vp, vp, dbl]
    L.nabo_community_destroy.argtypes = [vp]
    L.nabo_community_set_params.argtypes = [vp, dbl, C.c_uint64, i32, i32, i32]
    L.nabo_community_run.argtypes = [vp]
    L.nabo_community_labels.argtypes = [vp, vp, C.POINTER(i32), C.POINTER(dbl)]
    L.nabo_community_history.argtypes = [vp, C.POINTER(i64), i64, vp, vp]
    L.nabo_community_modularity.argtypes = [vp, vp, dbl, C.POINTER(dbl)]
    L.nabo_community_split.argtypes = [vp, vp, i32, vp, C.POINTER(i32)]
    L.nabo_community_level_size.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
    L.nabo_community_get_level.argtypes = [vp, vp, vp, vp, vp, vp]
    L.nabo_community_set_comm.argtypes = [vp, vp]
    L.nabo_community_get_comm.argtypes = [vp, vp]
    L.nabo_community_sweep.argtypes = [vp, i64, i64, C.POINTER(i64), C.POINTER(i64)]
    L.nabo_community_aggregate.argtypes = [vp]
    L.nabo_community_rewind.argtypes = [vp]
    L.nabo_community_last_ms.argtypes = [vp, C.POINTER(dbl)]
    L.nabo_community_geometry.argtypes = [C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.nabo_community_agglomerate.argtypes = [vp, i64]
    L.nabo_community_dendrogram.argtypes = [vp, C.POINTER(i64), i64, vp, vp]
    L.nabo_community_agglom_info.argtypes = [vp, C.POINTER(i64)]
    L.nabo_community_cut.argtypes = [vp, i64, vp, C.POINTER(i32), C.POINTER(dbl)]
    L.nabo_community_match_pass.argtypes = [vp, vp, vp, vp, vp]
    L.nabo_community_match.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), vp]
    L.nabo_community_agglom_ms.argtypes = [vp, C.POINTER(dbl)]
    L.nabo_potential_create.argtypes = [C.POINTER(vp), i32, i64, vp, vp]
    L.nabo_potential_destroy.argtypes = [vp]
    L.nabo_potential_set_params.argtypes = [vp, dbl, i64]
    L.nabo_potential_graph_size.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
    L.nabo_potential_prepare.argtypes = [vp, vp]
    L.nabo_potential_get_prepared.argtypes = [vp, vp, vp, vp, vp]
    L.nabo_potential_iterate.argtypes = [vp, i64, C.POINTER(i32)]
    L.nabo_potential_get_state.argtypes = [vp, vp, vp, vp, C.POINTER(dbl), C.POINTER(i64)]
    L.nabo_potential_set_state.argtypes = [vp, vp, vp, vp, dbl, i64]
    L.nabo_potential_finish.argtypes = [vp, vp]
    L.nabo_potential_solve.argtypes = [vp, vp, vp]
    L.nabo_potential_info.argtypes = [vp, C.POINTER(i64), C.POINTER(i32), C.POINTER(dbl), C.POINTER(dbl), C.POINTER(i64)]
    L.nabo_potential_last_ms.argtypes = [vp, C.POINTER(dbl)]
    L.nabo_potential_geometry.argtypes = [C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.nabo_bundle_create.argtypes = [C.POINTER(vp), i32, i64, vp, vp, i64, vp, vp]
    L.nabo_bundle_destroy.argtypes = [vp]
    L.nabo_bundle_set_params.argtypes = [vp, dbl, dbl, i32, i32, i32, i32, dbl, dbl, dbl, i32, i64]
    L.nabo_bundle_set_option.argtypes = [vp, C.c_char_p, i64]
    L.nabo_bundle_get_points.argtypes = [vp, C.POINTER(i64), vp, vp]
    L.nabo_bundle_set_points.argtypes = [vp, vp, vp]
    L.nabo_bundle_resample.argtypes = [vp]
    L.nabo_bundle_density.argtypes = [vp, vp]
    L.nabo_bundle_field.argtypes = [vp, dbl, vp, vp, vp]
    L.nabo_bundle_advect.argtypes = [vp, i64]
    L.nabo_bundle_smooth.argtypes = [vp, i64]
    L.nabo_bundle_run.argtypes = [vp]
    L.nabo_bundle_result.argtypes = [vp, vp, vp]
    L.nabo_bundle_last_ms.argtypes = [vp, C.POINTER(dbl)]
    L.nabo_bundle_geometry.argtypes = [C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.nabo_bundle_blur_weights.argtypes = [dbl, C.POINTER(i32), vp, i64]
    L.nabo_render_create.argtypes = [C.POINTER(vp), i32, i32, i32, dbl, dbl, dbl, dbl]
    L.nabo_render_destroy.argtypes = [vp]
    L.nabo_render_clear.argtypes = [vp]
    L.nabo_render_set_option.argtypes = [vp, C.c_char_p, i64]
    L.nabo_render_add_polylines.argtypes = [vp, i64, vp, vp]
    L.nabo_render_add_edges.argtypes = [vp, i64, vp, vp, i64, vp, vp]
    L.nabo_render_add_bundle.argtypes = [vp, vp]
    L.nabo_render_add_nodes.argtypes = [vp, i64, vp, vp, vp, vp]
    L.nabo_render_edge_counts.argtypes = [vp, vp]
    L.nabo_render_node_counts.argtypes = [vp, vp]
    L.nabo_render_node_sums.argtypes = [vp, vp]
    L.nabo_render_compose.argtypes = [vp, vp, vp, i32, vp, i32, vp]
    L.nabo_render_last_ms.argtypes = [vp, C.POINTER(dbl)]
    L.nabo_render_alpha_lut.argtypes = [dbl, i32, vp]
    L.nabo_render_geometry.argtypes = [C.POINTER(i32)] * 6
    L.nabo_mtx_create.argtypes = [i32, i64, i64, C.POINTER(vp)]
    L.nabo_mtx_feed.argtypes = [vp, vp, i64]
    L.nabo_mtx_finish.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
    L.nabo_mtx_get_csr.argtypes = [vp, vp, vp, vp]
    L.nabo_mtx_get_csc.argtypes = [vp, vp, vp, vp]
    L.nabo_mtx_free.argtypes = [vp]
    L.nabo_mtx_geometry.argtypes = [C.POINTER(i32), C.POINTER(i32)]
    L.nabo_mtx_last_device_ms.argtypes = [vp, C.POINTER(dbl), C.POINTER(i64)]
    L.nabo_csr_transpose.argtypes = [i32, i64, i64, vp, vp, vp, vp, vp, vp]
    L.nabo_mtxw_create.argtypes = [i32, i64, i64, vp, vp, vp, C.c_char_p, i32, i64, i64, C.POINTER(vp), C.POINTER(i64)]
    L.nabo_mtxw_read.argtypes = [vp, vp, i64, C.POINTER(i64)]
    L.nabo_mtxw_last_device_ms.argtypes = [vp, C.POINTER(dbl), C.POINTER(i64)]
    L.nabo_mtxw_free.argtypes = [vp]
    L.nabo_mtxw_geometry.argtypes = [C.POINTER(i32)] * 4
    L.nabo_counts_remap.argtypes = [i32, i64, i64, vp, vp, vp, i64, vp, i64, vp, C.POINTER(i64), vp, vp, vp, vp, vp, vp]
    L.nabo_csv_create.argtypes = [i32, i32, i64, i32, i32, i32, dbl, i64, i64, C.POINTER(vp)]
    L.nabo_csv_set_first_line.argtypes = [vp, i64]
    L.nabo_csv_feed.argtypes = [vp, vp, i64]
    L.nabo_csv_finish.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    L.nabo_csv_get_rows.argtypes = [vp, vp, vp, vp]
    L.nabo_csv_get_cols.argtypes = [vp, vp, vp, vp]
    L.nabo_csv_get_row_names.argtypes = [vp, vp, vp]
    L.nabo_csv_stats.argtypes = [vp, C.POINTER(i64)]
    L.nabo_csv_last_device_ms.argtypes = [vp, C.POINTER(dbl), C.POINTER(i64)]
    L.nabo_csv_geometry.argtypes = [C.POINTER(i32)] * 3
    L.nabo_csv_free.argtypes = [vp]
    for name in (SYMBOLS + GRAPH_SYMBOLS + CLUSTER_SYMBOLS + DE_SYMBOLS + PCA_SYMBOLS + PCA_FIT_SYMBOLS + QC_SYMBOLS + LAYOUT_SYMBOLS + UMAP_SYMBOLS
                 + UMAP_TRANSFORM_SYMBOLS + COMMUNITY_SYMBOLS + AGGLOM_SYMBOLS + POTENTIAL_SYMBOLS + BUNDLE_SYMBOLS + RENDER_SYMBOLS
                 + INGEST_SYMBOLS + COUNTS_SYMBOLS + CSV_SYMBOLS + INSPECT_SYMBOLS):
        if name not in ("nabo_version", "nabo_last_error", "nabo_layout_destroy", "nabo_umap_destroy", "nabo_umap_transform_destroy", "nabo_community_destroy",
                        "nabo_potential_destroy", "nabo_bundle_destroy", "nabo_render_destroy", "nabo_mtx_free", "nabo_mtxw_free", "nabo_csv_free"):
            getattr(L, name).restype = C.c_int
    _lib = L
    return L


def so_digest():
    """sha256 (first 16 hex digits) of the library file in use: bench.py prints it with every line"""
    import hashlib
    with open(SO_PATH, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


# sources a kernel's counter record depends on (profiles/pmc.json): the kernel, what it includes, the operand packing,
# the launch logic and the compiler flags
KERNEL_SOURCES = {
    "euclid": ["l2c_topk.hip", "l2q_topk.hip", "topk_lists.h", "knn_common.h", "pack.hip", "index.h", "plan.hip", "set_ref.hip", "query.hip", "api.hip", "_build.py",
               "local_seeds.hip", "local_seeds.h", "l2c_slots.h", "l2c_window.h", "bucket_order.hip", "bucket_order.h", "two_level_verdict.h",
               "bucket_skip.hip", "bucket_skip.h"],
    "canberra": ["canberra_f32.hip", "canberra_bits.hip", "knn_common.h", "index.h", "plan.hip", "set_ref.hip", "query.hip", "api.hip", "_build.py"],
}


def src_digest(names=None):
    """sha256 (first 16 hex digits) over sources the library is built from -- by default all of nabo_amd/csrc/*.hip,
    *.h, include/nabo_knn.h and nabo_amd/_build.py (the compiler flags); `names` restricts it (KERNEL_SOURCES).  Unlike
    the bytes of the .so it is the same after a rebuild on another box: profiles/pmc.json keys its records by it."""
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(HERE, "csrc")
    if names is None:
        files = sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".h")))
        files += [os.path.join(HERE, "..", "include", "nabo_knn.h"), os.path.join(HERE, "_build.py")]
    else:
        files = [os.path.join(HERE if f.endswith(".py") else csrc, f) for f in sorted(names)]
    for fn in files:
        h.update(os.path.basename(fn).encode())
        with open(fn, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def check(rc):
    """Map a C status to the reference's exception convention: bad parameters -> ValueError
    (nabo/_mapping.py:301,429,520,...), everything else -> NaboError."""
    if rc == 0:
        return
    msg = lib().nabo_last_error().decode("utf-8", "replace")
    if rc in (E_INVALID, E_UNSUPPORTED):
        raise ValueError("ERROR: " + msg)
    raise NaboError("nabo_knn error %d: %s" % (rc, msg))


def device_count():
    return int(lib().nabo_device_count())


def mem_info(device=0):
    """(free, total) bytes of the device's memory"""
    f, t = C.c_size_t(), C.c_size_t()
    check(lib().nabo_dev_mem_info(int(device), C.byref(f), C.byref(t)))
    return int(f.value), int(t.value)
