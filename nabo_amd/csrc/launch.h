// launch.h -- every function of libnabo_knn.so that one translation unit defines and another calls: the kernel launchers,
// their geometry and plan helpers, the index accessors sharded.hip uses, and the error recorder (what sharded.hip asks
// of comm.hip is declared in comm.h).  The defining file and
// every caller include it, so each definition is checked against the one declaration here; default arguments live here
// and nowhere else.  Host types only: tests/host_shim compiles comm.hip, sharded.hip and its fakes of some of these with g++.
#pragma once
#include <cstddef>
#include <cstdint>
#ifdef NABO_SHARDED_HOST
#include "hip_shim.h"
#else
#include <hip/hip_runtime.h>
#endif

struct nabo_index;     // index.h

namespace nabo {

// api.hip: records the message nabo_last_error() returns and passes the code through
int api_fail(int code, const char *fmt, ...);
// api.hip: what sharded.hip reads and sets on an index
int index_device(const nabo_index *ix);
int index_g(const nabo_index *ix);
int64_t index_n(const nabo_index *ix);
int index_metric(const nabo_index *ix);
bool index_can_emit_candidates(const nabo_index *ix);
void index_set_shard_mode(nabo_index *ix, bool on);
void index_set_cand_slack(nabo_index *ix, int s);

// pack.hip: fp32 tiles of the fp32-MFMA filter
hipError_t centre_launch(const double *Y, int64_t n, int g, double *centre, hipStream_t st);
hipError_t pack_ref_launch(const double *Y, int64_t n, int g, const double *centre, double scale, int ksteps, int64_t ntiles_total,
                           const uint8_t *mask, float *out, unsigned int *norm_max_bits, hipStream_t st);
hipError_t pack_query_launch(const double *X, int64_t m, int g, const double *centre, double scale, int ksteps,
                             int64_t ntiles_total, float *out, double *xnorm, hipStream_t st);
// f16 operands of the matrix-pipe filters (pack.hip): K-concatenated tiles, nseg = 3 the f16x3 split, 1 the one-product form
hipError_t maxabs_launch(const double *V, int64_t n, int g, const double *centre, unsigned long long *out_bits, hipStream_t st);
hipError_t pack_cref_launch(const double *Y, int64_t n, int g, const double *centre, double scale, int kc,
                            int64_t ntiles_total, const uint8_t *mask, unsigned char *out, unsigned int *norm_max_bits,
                            bool layout16, hipStream_t st, const uint32_t *perm = nullptr, int nseg = 3);
hipError_t pack_cquery_launch(const double *X, int64_t m, int g, const double *centre, double scale, int kc,
                              int64_t ntiles_total, unsigned char *out, double *xnorm, bool layout16, hipStream_t st,
                              const uint32_t *perm = nullptr, int nseg = 3);

// the fp32-MFMA filter (l2_topk.hip)
hipError_t l2_topk_launch(int ksteps, int epl, const float *Xpk, const float *Ypk, int tiles_per_split, int S, int gx,
                          int64_t tile_off, int lkeep, uint32_t *cand_idx, float *cand_key, float *cand_tau,
                          hipStream_t st);
void l2_topk_geometry(int ksteps, int epl, int *rows_per_wg, int *wg_per_cu, int *lkeep_max);
// the same filter on v_mfma_f32_16x16x32_f16 (l2q_topk.hip; operands packed with layout16)
int l2q_pick_kc(int g);
hipError_t l2q_topk_launch(int kc, const unsigned char *Xpk, const unsigned char *Ypk, int tiles_per_split, int S,
                           int gx, int64_t tile_off, int lkeep, uint32_t *cand_idx, float *cand_key, float *cand_tau,
                           int64_t pad_tile, hipStream_t st);
void l2q_topk_geometry(int kc, int *rows_per_wg, int *wg_per_cu, int *lkeep_max);
// the one-product first pass (l2c_topk.hip; operands packed with layout16, nseg = 1 or 2)
// A TWO-LEVEL launch (geometry B, two steps, operands in the two-level slot order): targets and references are bucket-ordered
// copies -- position p of the targets is the launch's row row_map[p] (0xFFFFFFFF: padding), position j of the stream is
// reference ref_map[j]; lists and seeds are indexed by the launch's rows, emitted candidates are reference indices.
// stats [4] (may be null): tiles run one-step, tiles of those refetched inside the loop (a segment's last tile, completed
// unconditionally, is not counted), tiles run two-step, tiles skipped (`runs`), summed over the waves.
// share_pct / burst: the mode control's refetch share and credit (0: the kernel's defaults).  bucket_end [nbucket] (may be
// null): the reference buckets' ends in tiles of the stream, non-decreasing (lseed_bucket_ends) -- the mode control keeps its
// account per bucket and runs two-step to a bucket's end.  stretch > 0, or no table: the control before that one, one
// account per one-step segment and blind two-step stretches, the first of `stretch` tiles (0: 64).
// window / check: the workgroup's progress window (l2c_window.h) -- a wave more than `window` tiles ahead of the slowest
// live wave of its workgroup waits, looking every `check` tiles (0: the defaults; window < 0: none).
// runs (may be null): per workgroup BSKIP_RUN_INTS int32 (bucket_skip.h), the stretches [begin, end) of the stream the
// workgroup runs, in order, even bounds, ended by the pair (0, 0) -- the tiles between them are skipped and counted in
// stats [3].  Null: the whole stream.
struct L2cOrdered {
    const uint32_t *row_map, *ref_map;
    unsigned long long *stats;
    int share_pct, stretch;
    const int32_t *bucket_end;
    int nbucket, burst;
    int window, check;
    const int32_t *runs;
};
int l2c_pick_kc(int g);
int l2c_geometry(int kc, int lkeep_want, int pin);
void l2c_topk_geometry(int kc, int lkeep_want, int pin, int *rows_per_wg, int *wg_per_cu, int *lkeep_max);
hipError_t l2c_topk_launch(int kc, int geo, const unsigned char *Xpk, const unsigned char *Ypk, int tiles_per_split, int S,
                           int gx, int64_t tile_off, int lkeep, uint32_t *cand_idx, float *cand_key, float *cand_tau,
                           int64_t pad_tile, hipStream_t st, int64_t rows_valid, const float *tau_init, int tau_stride = 0,
                           int64_t tau_row0 = 0, const struct L2cOrdered *ord = nullptr);
// tournament seeds for the one-product pass (l2c_topk.hip: l2c_pre_kernel)
void l2c_pre_plan(int kc, int lkeep, int tiles_per_split, int scale_pct, int *pre_tiles, int *gt);
hipError_t l2c_pre_launch(int kc, int lkeep, const unsigned char *Xpk, const unsigned char *Ypk, int tiles_per_split, int S,
                          int64_t rows, int64_t tile_off, int pre_tiles, int gt, int64_t pad_tile, hipStream_t st,
                          int64_t rows_valid, float *tau_out, const int *ranges = nullptr, int rows_per_col = 0,
                          const uint32_t *row_map = nullptr);
// local tournament seeds (local_seeds.hip; the layout rules: local_seeds.h)
size_t lseed_key_bytes(int64_t ncell);
size_t lseed_blockcnt_bytes(int64_t ncell, int C);
size_t lseed_layout_bytes(int C);
size_t lseed_anchor_bytes(int kc, int C);
// (two_level: the packed operands are in the two-level slot order, l2c_slots.h)
hipError_t lseed_anchors_launch(int kc, const unsigned char *Ypk, int64_t n, int g, int C, void *anchors, hipStream_t st,
                                bool two_level = false);
hipError_t lseed_sort_launch(int kc, bool is_ref, const unsigned char *pk, int64_t ncell, int g, const void *anchors, int C,
                             uint32_t *key, uint32_t *blockcnt, uint32_t *tot, hipStream_t st, bool two_level = false);
hipError_t lseed_fill_launch(int kc, const unsigned char *src, int64_t pad_cell, unsigned char *dst, int64_t ncell, hipStream_t st);
hipError_t lseed_layout_launch(int C, const uint32_t *ref_cnt, const uint32_t *row_cnt, int cap, int lkeep, int tile0,
                               const int rest[4], int64_t *lay, int *ranges, int64_t ncol, hipStream_t st);
hipError_t lseed_ends_launch(int C, const int64_t *lay, int32_t *end, hipStream_t st);
hipError_t lseed_move_launch(int kc, const unsigned char *src, int64_t ncell, const uint32_t *key, const uint32_t *blockoff, int C,
                             const int64_t *lay, int cap, int64_t pad_cell, unsigned char *dst, uint32_t *row_map, hipStream_t st);
// the sub-order inside the buckets of the two-level stream's copies (local_seeds.h): S sub-anchors per bucket, a second
// counting sort over a bucket-ordered copy (map1 [position] = cell, key1 [cell] >> 16 = bucket)
size_t lseed_sub_anchor_bytes(int kc, int C, int S);
size_t lseed_sub_float_bytes(int kc, int C, int S);
hipError_t lseed_sub_build_launch(int kc, const unsigned char *pk, const int64_t *lay, const uint32_t *ref_cnt, int g, int C, int S,
                                  bool by_index, void *anchors, float *subf, uint8_t *rank, float *norm, hipStream_t st, bool two_level);
hipError_t lseed_sub_sort_launch(int kc, bool is_ref, const unsigned char *pk, int64_t npos, const uint32_t *map1, const uint32_t *key1,
                                 const void *anchors, const float *norm, const uint8_t *rank, const uint32_t *ref_cnt, int C, int S,
                                 const int64_t *lay, uint32_t *key2, uint32_t *blockcnt, uint32_t *tot, int64_t *sublay, hipStream_t st);
hipError_t lseed_sub_move_launch(int kc, const unsigned char *src, int64_t npos, const uint32_t *map1, const uint32_t *key2,
                                 const uint32_t *blockoff, const int64_t *sublay, const unsigned char *pad_src, int64_t pad_cell, int C,
                                 const int64_t *lay, unsigned char *dst, uint32_t *dst_map, hipStream_t st);
// the sub-buckets a workgroup of the ordered main launch cannot need (bucket_skip.hip; the rule: bucket_skip.h)
size_t bskip_dir_bytes(int C, int g);
size_t bskip_mean_part_bytes(int C, int g);
hipError_t bskip_refs_launch(const double *Y, const double *centre, double scale, int g, int C, int S, const int64_t *lay,
                             const uint32_t *ref_cnt, const int64_t *sublay, const uint32_t *subtot, const uint32_t *ref_map,
                             int32_t *first, int32_t *count, int32_t *t0, int32_t *t1, double *mean_parts, double *mean, double *by_from,
                             double *by_to, float *ymin, hipStream_t st);
hipError_t bskip_runs_launch(const double *X, const double *centre, double scale, int g, int C, int S, const uint32_t *row_map,
                             const uint32_t *key, const float *tau, const double *by_from, const float *ymin, const int32_t *t0,
                             const int32_t *t1, int64_t t_end, int64_t wgs, int32_t *runs, hipStream_t st);

// list merges, float64 re-evaluation, exact kernels and row helpers (refine.hip)
hipError_t merge_lists_launch(const uint32_t *cand_idx, const float *cand_key, const float *cand_tau, int64_t rows, int S, int L,
                              int lkeep, int Lout, uint32_t *out_idx, float *out_tau, hipStream_t st);
hipError_t pairwise_launch(const double *X, int64_t m, const double *Y, int64_t n, int g, int metric, double f,
                           double *D, hipStream_t st);
hipError_t refine_launch(const double *X, int64_t row0, int64_t m, const double *Y, int g, const uint32_t *cand_idx,
                         const float *cand_tau, int S, int L, const double *xnorm, double err_coef, double ymax_sqrt,
                         double tau_scale, int k, int drop, int64_t base, int64_t n_valid_total, const uint32_t *masked_list,
                         int n_masked_list, int64_t *out_idx, double *out_dist, uint32_t *fail_rows,
                         unsigned int *fail_count, hipStream_t st, int metric = 0, double cb_f = 0.0,
                         float cb_plateau = 0.0f, int lvalid = 0, const uint32_t *rperm = nullptr,
                         const uint32_t *tperm = nullptr, float *fail_seed = nullptr);
hipError_t refine_cand_launch(const double *X, int64_t row0, int64_t m, const double *Y, int g, const uint32_t *cand_idx,
                              const float *cand_tau, int S, int L, const double *xnorm, double err_coef,
                              double ymax_sqrt, double tau_scale, int kout, int64_t base, int64_t n_valid_total,
                              int64_t *out_idx, double *out_dist, double *out_bound, hipStream_t st, int metric = 0,
                              int lvalid = 0, const uint32_t *rperm = nullptr, const uint32_t *tperm = nullptr);
hipError_t normalise_rows_launch(const double *X, int64_t m, int g, double *out, hipStream_t st);
hipError_t exact_rows_launch(const double *X, const double *Y, int64_t n, int g, int metric, double f,
                             const uint8_t *mask, const uint32_t *rows, unsigned int nrows, int k, int drop,
                             int64_t base, const uint32_t *masked_list, int n_masked_list, int64_t *out_idx,
                             double *out_dist, double *D, unsigned int d_rows, hipStream_t st);
hipError_t masked_tail_launch(const double *X, int64_t m, const double *Y, int g, int metric, double f,
                              const uint32_t *masked_list, int n_masked_list, int n_valid, int k, int drop,
                              int64_t base, int64_t *out_idx, double *out_dist, hipStream_t st);
hipError_t gather_rows_launch(const double *X, const uint32_t *rows, int64_t nrows, int g, double *out, hipStream_t st);
hipError_t iota_launch(uint32_t *out, int64_t n, hipStream_t st);
hipError_t scatter_rows_launch(const int64_t *si, const double *sd, const uint32_t *rows, int64_t nrows, int k,
                               int64_t *out_idx, double *out_dist, hipStream_t st);

// exact Canberra kernel, the top-k merges and SNN counts (canberra.hip)
hipError_t transpose_ref_launch(const double *Y, int64_t n, int g, double *Yt, hipStream_t st);
hipError_t canberra_topk_launch(int epl, const double *X, int64_t m, const double *Yt, int64_t n, int g, double f,
                                const uint8_t *mask, int S, double *cand_d, uint32_t *cand_i, hipStream_t st);
hipError_t merge_local_launch(const double *cand_d, const uint32_t *cand_i, int64_t m, int P, int k, int drop,
                              int64_t base, int64_t *out_idx, double *out_dist, int *n_found, hipStream_t st);
hipError_t merge_parts_launch(const double *parts_d, const int64_t *parts_i, int n_parts, int64_t m, int kp, int k,
                              int drop, int64_t *out_idx, double *out_dist, hipStream_t st);
hipError_t snn_counts_launch(const int64_t *t_idx, int64_t m, const int64_t *r_idx, int64_t n, int k, int32_t *out,
                             hipStream_t st);

// fp32 lower-bound Canberra filter (canberra_f32.hip)
hipError_t cbf_pack_targets_launch(const double *X, int64_t m, int g, int gp, double f, float *xq, unsigned int *flag,
                                   hipStream_t st);
hipError_t cbf_pack_refs_launch(const double *Y, int64_t n, int g, int gp, float *ycf, unsigned int *flag,
                                hipStream_t st);
int cbf_pick_gp(int g);
void cbf_constants(int g, float *slack, float *plateau);
int cbf_lists_per_split();
int cbf_rows_per_wg(int epl);
hipError_t cbf_filter_launch(int gp, int epl, const float *xq, const void *xh, int64_t m, const float *ycf,
                             const void *ych, int64_t n, int g, const uint8_t *mask, int S, uint32_t *cand_idx,
                             float *cand_tau, hipStream_t st);
hipError_t cbf_pack_refs_rows_launch(const double *Y, int64_t n, int g, int gp, float *yrow, hipStream_t st);
hipError_t cbf_colminmax_launch(const double *Y, int64_t n, int g, unsigned int *colmm, hipStream_t st);
hipError_t cbf_pack_refs8_launch(const double *Y, int64_t n, int g, int gp, const double *quant, void *ych, hipStream_t st);
hipError_t cbf_pack_targets8_launch(const double *X, int64_t m, int g, int gp, double f, const double *quant, void *xh,
                                    hipStream_t st);
// the counting pass on per-bucket bitmaps (canberra_bits.hip)
int cbb_buckets();
int cbb_rows_per_wg();
bool cbb_available(int g, int gp, int epl);
size_t cbb_table_bytes(int64_t n, int g);
size_t cbb_valid_bytes(int64_t n);
hipError_t cbb_pack_table_launch(const double *Y, int64_t n, int g, const double *edges, uint32_t *tab, hipStream_t st);
hipError_t cbb_valid_launch(const uint8_t *mask, int64_t n, uint32_t *vbits, hipStream_t st);
hipError_t cbb_pack_targets_launch(const double *X, int64_t m, int g, int gp, double f, const double *edges, uint16_t *rowoff,
                                   hipStream_t st);
hipError_t cbb_filter_launch(int gp, const float *xq, const uint16_t *rowoff, int64_t m, const float *yrow, const uint32_t *tab,
                             const uint32_t *vbits, int64_t n, int g, int S, uint32_t *cand_idx, float *cand_tau, hipStream_t st);

// COO edges -> CSR by reference node, a stable device sort (csr_build.hip; for score_null.hip)
hipError_t csr_sort_temp_bytes(int64_t E, int64_t n_ref, size_t *bytes);
hipError_t csr_build_launch(const int64_t *edge_r, const int64_t *edge_t, const double *edge_w, int64_t E, int64_t n_ref,
                            int64_t n_t, uint32_t *keys_a, uint32_t *pos_a, uint32_t *keys_b, uint32_t *pos_b, void *temp,
                            size_t temp_bytes, int64_t *row_ptr, int64_t *out_t, double *out_w, unsigned int *flag,
                            hipStream_t st);
// sorted (row << 32 | column) keys, row n for a key that is no arc -> ptr [n + 1]; and the bits their radix sort needs (csr_build.hip)
hipError_t key_rowptr_launch(const uint64_t *keys, int64_t n_keys, int64_t n, int64_t *ptr, hipStream_t st);
unsigned key_sort_bits(int64_t n);
// sorted 32-bit keys in [0, n) -> ptr [n + 1], ptr[r] = the first position whose key is >= r; E = 0 is allowed (csr_build.hip)
hipError_t u32_rowptr_launch(const uint32_t *keys, int64_t E, int64_t n, int64_t *ptr, hipStream_t st);

// Matrix Market text -> entries in file order, and the sorts that make the two indexes of them (mtx_ingest.hip).
// One piece of whole lines: text [len] (readable up to a whole 16 bytes), one workgroup per tile of n_tiles =
// ceil(len / tile); stage_key / stage_val [n_tiles * mtx_tile_entries()], tile_count and tile_base [n_tiles + 1];
// the piece's entries go to out_key / out_val [nnz] from position `done` on (those at or past nnz are dropped);
// tile_base[n_tiles] is their number and res the lowest bad line and the number of lines.
struct MtxPieceResult {
    unsigned long long err;      // min over the bad lines of (byte offset of the line in the piece << 8 | code); ~0: none
    unsigned long long n_lines;
};
int mtx_tile_entries();
hipError_t mtx_scan_temp_bytes(int64_t n_tiles, size_t *bytes);
hipError_t mtx_parse_launch(const uint8_t *text, int64_t len, int64_t n_genes, int64_t n_cells, uint64_t *stage_key, uint32_t *stage_val,
                            uint32_t *tile_count, uint32_t *tile_base, void *temp, size_t temp_bytes, int64_t done, int64_t nnz,
                            uint64_t *out_key, uint32_t *out_val, MtxPieceResult *res, hipStream_t st);
// (major << 32 | minor) keys with 4-byte values, both double-buffered (a: the data, b: scratch; which: 0 / 1, the buffer
// that holds the data, updated): sorted by the minor's bits [0, bits(n_minor)) alone (STABLE) and, with_major, by the
// major's bits after that
hipError_t mtx_sort_temp_bytes(int64_t nnz, int64_t n_major, int64_t n_minor, size_t *bytes);
hipError_t mtx_sort_launch(uint64_t *key[2], uint32_t *val[2], int *which, int64_t nnz, int64_t n_major, int64_t n_minor, bool with_major,
                           void *temp, size_t temp_bytes, hipStream_t st);
// *dup = the lowest key that equals its left neighbour (~0: none)
hipError_t mtx_dup_launch(const uint64_t *keys, int64_t nnz, unsigned long long *dup, hipStream_t st);
// lo[i] = the low, hi[i] = the high half of keys[i]; either may be NULL
hipError_t mtx_split_launch(const uint64_t *keys, int64_t nnz, uint32_t *lo, uint32_t *hi, hipStream_t st);
// keys[e] = row of e << 32 | idx[e] for the entries of a CSR
hipError_t mtx_expand_launch(const int64_t *ptr, int64_t n_rows, const int32_t *idx, int64_t nnz, uint64_t *keys, hipStream_t st);

// differential expression: keys of a gene chunk, their sort and the rank kernel (de_rank.hip)
hipError_t de_temp_bytes(int64_t nnz_max, int64_t keys_max, int64_t n_seg, size_t *bytes);
hipError_t de_expand_launch(const int32_t *cell, const float *val, int64_t nnz, const int64_t *gptr, int32_t n_genes_chunk,
                            const float *sf, const int64_t *inv_ptr, const int32_t *inv_set, int64_t n_sets, uint32_t *cnt,
                            uint32_t *off, void *temp, size_t temp_bytes, uint64_t *keys, int64_t key_base, hipStream_t st);
hipError_t de_sort_launch(const uint64_t *keys_a, uint64_t *keys_b, int64_t n_keys, int64_t n_seg, void *temp, size_t temp_bytes,
                          int64_t *seg, hipStream_t st);
hipError_t de_rank_launch(const uint64_t *keys, const int64_t *seg, int64_t n_sets, const int64_t *set_size, int64_t n_pairs,
                          const int32_t *pair_test, const int32_t *pair_ctrl, int64_t n_genes_chunk, double exp_frac_thresh,
                          double log2_fc_thresh, int32_t *out_status, int64_t *out_i64, double *out_f64, hipStream_t st);

// PCA projection of sparse cells and per-gene statistics (pca_project.hip)
hipError_t pca_project_launch(const int64_t *ptr, const int32_t *gene, const float *val, const float *sf_row, int64_t n_rows,
                              const int32_t *gene_pos, const double *sigma, const double *bias, const double *Tt, int C, double *Z,
                              hipStream_t st);
hipError_t gene_stats_launch(const int64_t *gptr, const int32_t *cell, const float *val, const float *sf, const uint8_t *kept,
                             const uint8_t *keep_gene, int64_t n_genes, int64_t n_keep, int64_t *out_ncells, uint8_t *out_valid,
                             double *out_m, double *out_nzm, double *out_var, hipStream_t st);

// the exact PCA fit: dense centred rows, their column sums and Y^T Y by f64 MFMA (pca_fit.hip)
int pca_fit_tile();                     // genes per side of an output tile; a row of the chunk holds a multiple of it
int pca_fit_row_pad();                  // the chunk holds a multiple of this many rows
int pca_fit_splits(int64_t n_tiles);    // partial tiles per tile, at most
int pca_fit_sum_slices();               // partial column sums per column, at most
hipError_t pca_densify_launch(const int64_t *ptr, const int32_t *gene, const float *val, const float *sf_row, int64_t n_rows, int64_t n_rows_pad,
                              const int32_t *gene_pos, const double *mu, const double *sigma, const double *fill, const double *mean, int G,
                              int Gp, double *Y, hipStream_t st);
hipError_t pca_colsum_launch(const double *Y, int64_t n_rows, int Gp, double *partial, double *colsum, hipStream_t st);
hipError_t pca_syrk_launch(const double *Y, int64_t n_rows_pad, int Gp, double *partial, double *acc, hipStream_t st);
hipError_t pca_cov_finish_launch(const double *acc, int G, int64_t n, double *cov, hipStream_t st);
// the host check the projection and the fit share, and what nabo_pca_last_device_ms reports (pca_project.hip)
int pca_check_selection(int64_t n_raw_genes, const int32_t *gene_pos, int64_t G, const double *sigma, int64_t n_cells, int64_t n_rows,
                        const int64_t *rows);
void pca_set_device_ms(const double ms[3], int64_t n_chunks);

// per-cell quality-control sums: one streaming pass over the cells (cell_qc.hip); table: the class bytes, padded with
// zeros to a multiple of 16
hipError_t cell_qc_launch(const int64_t *ptr, const int32_t *gene, const float *val, int64_t n_rows, const uint8_t *table,
                          int64_t n_raw_genes, int n_classes, int64_t *out_n, double *out_sums, hipStream_t st);

// device time of the last classification / set-levels call, read by nabo_cluster_last_device_ms (classify.hip)
void cluster_set_device_ms(int which, double ms);

// ForceAtlas2 layout, one iteration = these five in this order (layout.hip; include/nabo_layout.h has the definition).
// LayoutScalars lives on the device: the speed kernel's single thread writes it, every later kernel reads it, and once
// `stop` is set (S == 0 or T == 0) every kernel but pack returns at once.
struct LayoutScalars {
    double speed, eff, S, T;
    long long done;   // iterations that moved the nodes
    int stop, pad_;
};
struct LayoutParams {
    double scaling_ratio, gravity, comp;   // comp: mean(mass) with outbound attraction distribution, else 1
    int oad, strong;
};
int layout_iblock();   // nodes i per workgroup of the repulsion kernel; pk holds a multiple of it
int layout_jtile();    // nodes j per staged tile
hipError_t layout_pack_launch(const double *x, const double *y, const double *mass, int64_t n, int64_t npad, void *pk, hipStream_t st);
// part: [n_splits][2][n] (nabo_layout_geometry gives n_splits)
hipError_t layout_repulse_launch(const void *pk, int64_t n, double *part, const LayoutScalars *sc, hipStream_t st);
hipError_t layout_node_launch(int64_t n, const double *x, const double *y, const double *mass, double *dx, double *dy,
                              const int64_t *ptr, const int32_t *nbr, const double *ew, const double *part, const LayoutParams &P,
                              double *f_rep, double *f_grav, double *f_attr, double *swing, double *block_st,
                              const LayoutScalars *sc, hipStream_t st);
hipError_t layout_speed_launch(int64_t n, const double *block_st, double jitter_tolerance, LayoutScalars *sc, hipStream_t st);
hipError_t layout_move_launch(int64_t n, double *x, double *y, const double *dx, const double *dy, const double *swing,
                              LayoutScalars *sc, hipStream_t st);

// UMAP embedding (umap.hip; include/nabo_umap.h has the definition).  The graph build is smooth -> graph -> arcs; one
// epoch is one launch of the epoch kernel, which reads y and writes ynew.
struct UmapEpoch {
    double a, b, ca, cr;      // the curve; ca = (-2 a) b, cr = (2 gamma) b
    double alpha, t;          // this epoch's step length and number
    uint64_t s_t;             // mix(seed + G (t + 1)): the epoch's part of the negative-sample hash
};
int umap_group();             // lanes per node of the epoch kernel
hipError_t umap_smooth_launch(const double *dist, int64_t n, int k, double target, double *rowsum, double *rho, double *total,
                              double *sigma, hipStream_t st);
hipError_t umap_sort_temp_bytes(int64_t n_slots, int64_t n, size_t *bytes);
// keys_*, w_*: [2 n k] slots; on return keys_b, w_b hold the pruned arcs in CSR order and ptr[n] their number
hipError_t umap_graph_launch(const int64_t *idx, const double *dist, int64_t n, int k, const double *rho, const double *sigma,
                             double n_epochs, double *a, uint64_t *keys_a, double *w_a, uint64_t *keys_b, double *w_b, void *temp,
                             size_t temp_bytes, double *wmax, int64_t *ptr, hipStream_t st);
// nbr may be NULL (the schedule alone is set back to its first state)
hipError_t umap_arcs_launch(const uint64_t *keys, const double *w, int64_t n_arcs, const double *wmax, double nsr, int32_t *nbr,
                            double *eps, double *epn, double *next, double *nneg, hipStream_t st);
hipError_t umap_epoch_launch(int dims, int64_t n, const int64_t *ptr, const int32_t *nbr, const double *eps, const double *epn,
                             double *next, double *nneg, const double *y, double *ynew, const UmapEpoch &P, int32_t *n_attr,
                             int32_t *n_neg, uint64_t *idx_sum, hipStream_t st);

// UMAP transform (umap_transform.hip; include/nabo_umap_transform.h has the definition).  A batch is graph -> schedule;
// one run is ONE launch of the optimise kernel over the epochs [t0, t1): the reference positions Y are only read.
struct UmapTransformRun {
    double a, b, ca, cr;      // the curve; ca = (-2 a) b, cr = (2 gamma) b
    double n_epochs, nsr;     // as float64
    int64_t t0, t1;           // the epochs of this run
    uint64_t seed;
    int64_t first_row;        // the global number of the batch's row 0: part of the negative-sample hash
    int64_t n_ref;
};
int umap_transform_group();   // lanes per target of the optimise kernel
// dist NULL: memb [m][k] is given (sigma = 0); else B' and C' from dist.  Then the start y0 and y = y0.
hipError_t umap_transform_graph_launch(int dims, int64_t m, int k, const int64_t *idx, const double *dist, const double *Y,
                                       double *sigma, double *memb, double *y0, double *y, hipStream_t st);
hipError_t umap_transform_schedule_launch(int64_t mk, const double *memb, double n_epochs, double nsr, double *next, double *nneg,
                                          hipStream_t st);
hipError_t umap_transform_run_launch(int dims, int64_t m, int k, const int64_t *idx, const double *memb, double *next, double *nneg,
                                     const double *Y, double *y, const UmapTransformRun &P, int64_t *n_attr, int64_t *n_neg,
                                     uint64_t *idx_sum, hipStream_t st);

// Communities of the reference graph (community.hip; include/nabo_community.h has the definition).  One sweep is
// totsize then sweep, which reads comm and writes comm_new; an aggregation is totsize, renumber, part_sums with keys,
// coarse_sort, key_rowptr, coarse_arcs and compose.
struct CommunitySweep {
    double gamma, two_m;      // the resolution and 2m as a double
    uint64_t h2;              // mix(mix(seed + G (L + 1)) + G (s + 1)): the gate's part of (level, sweep)
};
int community_huge_blocks();       // dense tables of the global-memory path; scratch holds this many times n entries, zeroed
hipError_t community_totsize_launch(int64_t n, const int32_t *comm, const int64_t *k, int64_t *tot, int32_t *size, hipStream_t st);
// counters: {moved, want}, added to; long_rows, ovf [n_long], ovf_count, scratch: unused when n_long == 0
hipError_t community_sweep_launch(int64_t n, const int64_t *ptr, const int32_t *nbr, const int64_t *a, const int64_t *k, const int32_t *comm,
                                  const int64_t *tot, const int32_t *size, const CommunitySweep &P, const int32_t *long_rows, int64_t n_long,
                                  int32_t *ovf, unsigned int *ovf_count, int64_t *scratch, int32_t *comm_new, uint64_t *counters,
                                  hipStream_t st);
hipError_t community_renumber_temp_bytes(int64_t n, size_t *bytes);
// flag[c] = community c is used, newid = its exclusive prefix sum, lab[i] = newid[comm[i]]
hipError_t community_renumber_launch(int64_t n, const int32_t *size, const int32_t *comm, int32_t *flag, int32_t *newid, int32_t *lab, void *temp,
                                     size_t temp_bytes, hipStream_t st);
// d[c] = sum of k, in2[c] = sum of in plus the inner arcs, c = lab[i] in [0, n_next); keys, vals (may be NULL): [A]
hipError_t community_part_sums_launch(int64_t n, int64_t A, const int32_t *src, const int32_t *nbr, const int64_t *a, const int64_t *k,
                                      const int64_t *inn, const int32_t *lab, int64_t n_next, int64_t *d, int64_t *in2, uint64_t *keys,
                                      int64_t *vals, hipStream_t st);
hipError_t community_coarse_temp_bytes(int64_t A, int64_t n_next, size_t *bytes);
hipError_t community_coarse_sort_launch(int64_t A, int64_t n_next, const uint64_t *keys_a, const int64_t *vals_a, uint64_t *keys_b,
                                        int64_t *vals_b, uint64_t *ukeys, int64_t *usums, int64_t *n_unique, void *temp, size_t temp_bytes,
                                        hipStream_t st);
// src, nbr of the A >= 1 coarse arcs, the first A of the sorted keys (A = ptr[n_next] of key_rowptr_launch)
hipError_t community_coarse_arcs_launch(const uint64_t *ukeys, int64_t A, int32_t *src, int32_t *nbr, hipStream_t st);
hipError_t community_compose_launch(int64_t n, int32_t *map, const int32_t *lab, hipStream_t st);
// one round of the component split: hook, then pointer jumping; *changed != 0 if a label fell
hipError_t community_hook_launch(int64_t n, int64_t A, const int32_t *src, const int32_t *nbr, const int32_t *part, int32_t *lab,
                                 int32_t *changed, hipStream_t st);
// pointer jumping alone: lab[i] = the end of the chain i -> lab[i] -> ... (every chain must end at a fixed point)
hipError_t community_jump_launch(int64_t n, int32_t *lab, hipStream_t st);

// Greedy modularity agglomeration (agglom.hip; include/nabo_agglom.h has the definition).  A round is passes of
// pass + mark until a pass matches nothing, then select + sort (or first, in the round without a positive gain), records,
// comm, the aggregation of community.hip and rep.
int agglom_group();                // lanes per row of the pass's short path
// one pass over the free rows: partner (-1: none), the winning D as (dhi, dlo) and its arc's weight wa, all [n]; rows that
// are not free are left alone.  long_rows [n_long]: the rows of more than long_threshold arcs.  any_sign: D <= 0 counts too
hipError_t agglom_pass_launch(int64_t n, const int64_t *ptr, const int32_t *nbr, const int64_t *a, const int64_t *k, const uint8_t *free,
                              int64_t two_m, int long_threshold, const int32_t *long_rows, int64_t n_long, bool any_sign, int32_t *partner,
                              int64_t *dhi, uint64_t *dlo, int64_t *wa, hipStream_t st);
// clears free at mutual picks and adds the number of new pairs to *counter
hipError_t agglom_mark_launch(int64_t n, const int32_t *partner, uint8_t *free, uint64_t *counter, hipStream_t st);
// sel[0] = the lower end of the first pair of the order over every row's pick (partner[sel[0]] is its other end)
hipError_t agglom_first_launch(int64_t n, const int32_t *partner, const int64_t *dhi, const uint64_t *dlo, int32_t *sel, hipStream_t st);
hipError_t agglom_order_temp_bytes(int64_t n, size_t *bytes);
// sel = the lower ends of the matched pairs in ascending id, *count (device) how many; flag [n]: scratch
hipError_t agglom_select_launch(int64_t n, const int32_t *partner, const uint8_t *free, int32_t *flag, int32_t *sel, size_t *count, void *temp,
                                size_t temp_bytes, hipStream_t st);
// sel_a [m] in ascending id -> sel_a in pair order (every D > 0); sel_b, key_a, key_b [m]: scratch
hipError_t agglom_sort_launch(int64_t m, const int64_t *dhi, const uint64_t *dlo, int32_t *sel_a, int32_t *sel_b, uint64_t *key_a,
                              uint64_t *key_b, void *temp, size_t temp_bytes, hipStream_t st);
// rec [m][6] = (rep_a, rep_b, round, a_cd, k_a, k_b), pairs [m][2] = (c, d); either may be NULL
hipError_t agglom_records_launch(int64_t m, const int32_t *sel, const int32_t *partner, const int64_t *wa, const int64_t *k, const int32_t *rep,
                                 int64_t round, int64_t *rec, int32_t *pairs, hipStream_t st);
// comm (the identity beforehand): comm[d] = c for the first `take` pairs
hipError_t agglom_comm_launch(int64_t take, const int32_t *sel, const int32_t *partner, int32_t *comm, hipStream_t st);
// flag, newid: of the aggregation's renumbering; rep_next[newid[c]] = rep[c] for every surviving c
hipError_t agglom_rep_launch(int64_t n, const int32_t *flag, const int32_t *newid, const int32_t *rep, int32_t *rep_next, hipStream_t st);
// parent[rep_b[i]] = rep_a[i], i < t
hipError_t agglom_parent_launch(int64_t t, const int32_t *rep_a, const int32_t *rep_b, int32_t *parent, hipStream_t st);

}  // namespace nabo
