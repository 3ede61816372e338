"""nabo_amd -- MI355X-native k-NN mapping hot path behind Nabo's Mapping API.

Public names mirror the reference's `nabo` package for this path (`Mapping`), plus the
array-level entry points of the C ABI (`knn`, `pairwise`, `KnnIndex`)."""
from ._lib import EUCLIDEAN, MOD_CANBERRA, COSINE, NaboError, device_count  # noqa: F401
from ._knn import knn, knn_devices, pairwise, KnnIndex, snn_counts  # noqa: F401
from ._mapping import Mapping, write_dense_pca, expand_graph  # noqa: F401
from ._score import (get_mapping_score, mapping_score_from_edges, mapping_score_null,  # noqa: F401
                     get_mapping_score_null)
from ._paths import (RefGraph, group_hops, get_mapping_specificity, get_ref_specificity,  # noqa: F401
                     calc_contiguous_spl)
from ._classify import (classify_target, classify_from_edges, get_k_path_neighbours, get_de_groups,  # noqa: F401
                        get_mapped_cells)
from ._de import de_test_csc, run_de_test, find_cluster_markers  # noqa: F401
from ._pca import pca_project_csr, gene_stats_csc, get_scaling_params, transform_pca  # noqa: F401
from ._pca import pca_cov_csr, fit_pca_csr, fit_pca, FittedPCA  # noqa: F401
from ._qc import (cell_qc_csr, filter_data, set_sf, qc_and_sf, gene_stats, correct_var, find_hvgs, get_lvgs,  # noqa: F401
                  dump_hvgs)
from ._layout import layout_fa2, set_ref_layout, save_layout_as_json, save_layout_as_csv  # noqa: F401
from ._umap import make_umap, umap_fit, umap_fuzzy_graph, find_ab_params, Umap  # noqa: F401
from ._umap import make_target_umap, umap_transform, UmapTransform  # noqa: F401
from ._community import (louvain_csr, modularity_csr, Community, make_leiden_clusters, calc_modularity,  # noqa: F401
                         save_clusters_as_json, save_clusters_as_csv, agglomerate_csr, make_clusters)
from ._potential import diff_potential_csr, Potential, calc_diff_potential  # noqa: F401
from ._bundle import Bundle, hammer_bundle, bundle_edges  # noqa: F401
from ._render import (Canvas, render_graph, plot_graph, draw_image, vertex_colors, vertex_radii, centroid_labels,  # noqa: F401
                      alpha_lut, default_viewport)
from ._ingest import MtxReader, CountMatrix, read_mtx, mtx_to_h5, csr_to_csc, fix_dup_names  # noqa: F401
from ._counts import (MtxWriter, write_mtx, remap_counts, read_h5_counts, subset_cells, merge_counts,  # noqa: F401
                      extract_cells_from_h5, merge_h5, h5_to_mtx)
from ._csv import CsvReader, CsvMatrix, read_csv, csv_to_h5  # noqa: F401

__all__ = ["CsvReader", "CsvMatrix", "read_csv", "csv_to_h5","MtxWriter", "write_mtx", "remap_counts", "read_h5_counts", "subset_cells", "merge_counts", "extract_cells_from_h5", "merge_h5", "h5_to_mtx", "MtxReader", "CountMatrix", "read_mtx", "mtx_to_h5", "csr_to_csc", "fix_dup_names", "Canvas", "render_graph", "plot_graph", "draw_image", "vertex_colors", "vertex_radii", "centroid_labels", "alpha_lut", "default_viewport", "Bundle", "hammer_bundle", "bundle_edges", "diff_potential_csr", "Potential", "calc_diff_potential", "louvain_csr", "modularity_csr", "Community", "make_leiden_clusters", "calc_modularity", "save_clusters_as_json", "save_clusters_as_csv", "agglomerate_csr", "make_clusters", "make_umap", "umap_fit", "umap_fuzzy_graph", "find_ab_params", "Umap", "make_target_umap", "umap_transform", "UmapTransform", "layout_fa2", "set_ref_layout", "save_layout_as_json", "save_layout_as_csv", "cell_qc_csr", "filter_data", "set_sf", "qc_and_sf", "gene_stats", "correct_var", "find_hvgs", "get_lvgs", "dump_hvgs", "pca_project_csr", "gene_stats_csc", "get_scaling_params", "transform_pca", "pca_cov_csr", "fit_pca_csr", "fit_pca", "FittedPCA", "de_test_csc", "run_de_test", "find_cluster_markers", "classify_target", "classify_from_edges", "get_k_path_neighbours", "get_de_groups", "get_mapped_cells", "Mapping", "write_dense_pca", "expand_graph", "get_mapping_score", "mapping_score_from_edges", "mapping_score_null", "get_mapping_score_null", "RefGraph", "group_hops", "get_mapping_specificity", "get_ref_specificity", "calc_contiguous_spl", "knn", "knn_devices", "pairwise", "KnnIndex", "snn_counts", "device_count", "EUCLIDEAN", "MOD_CANBERRA", "COSINE",
           "NaboError"]
