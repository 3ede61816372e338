/*
 * nabo_umap_transform.h -- C ABI of the UMAP transform in libnabo_knn.so (MI355X, gfx950): target cells placed in a
 * fitted reference embedding that does not move.
 *
 * What umap-learn 0.5 users call UMAP.transform.  The definition below is the specification; umap-learn's own
 * floating-point results and its random stream are not pinned.  It follows umap-learn's transform part
 * by part; the deliberate differences are listed after it.  Same conventions as nabo_umap.h: 0 or a negative NABO_E_*
 * status, the message in nabo_last_error(), no CPU fallback (NABO_E_NODEVICE without a device).  Every pointer is a host
 * pointer.
 *
 * THE DEFINITION.  Everything is float64 unless said otherwise, no operation is fused.  TREE, mix, clip and
 * G = 0x9E3779B97F4A7C15 mean what they mean in nabo_umap.h.
 *
 * The reference: n_ref cells with fitted positions Y [n_ref][dims], dims 2 or 3, n_ref < 2^31.  A batch is m target rows
 * that carry the global row numbers first_row .. first_row + m - 1.
 *
 * A'. Neighbours.  idx[m][k], dist[m][k]: each target's k nearest REFERENCE cells in (dist asc, idx asc) order -- what
 *     nabo_index_query returns for the targets against the reference with drop_first = 0.  2 <= k <= NABO_MAX_K,
 *     k <= n_ref.
 *
 * B'. Smooth distances, with umap's local_connectivity - 1 = 0:
 *       rho_i   = 0.
 *       psum(m) = part B's with rho = 0: TREE(v), v_0 = 0 and for t = 1 .. k-1: v_t = 1 if d_t <= 0, else
 *                 exp(-(d_t / m)).  Position 0 is skipped, as umap skips it, although it is a real neighbour here.
 *       sigma_i : part B's 64-step search, word for word (target = log2(k); lo = 0, hi = inf, mid = 1; ...).
 *       floor   : sigma_i = max(sigma_i, 1e-3 * (TREE(d_0 .. d_{k-1}) / k)) -- the row's own mean.
 *
 * C'. Memberships.  For every position t = 0 .. k-1:
 *       a_it = 1 if d_it <= 0 or sigma_i == 0, else exp(-(d_it / sigma_i)).
 *     There is no self entry and no union.  Arc (i, t) is LIVE iff a_it >= 1 / n_epochs (n_epochs as float64).
 *
 *     Start.  s_i = TREE(a_i0 .. a_i,k-1);  y_i = the sum over t = 0 .. k-1, in that order and starting from 0, of
 *     (a_it / s_i) * Y[idx_it], per component.
 *
 * D'. Epochs.  Per live arc: eps = 1 / a_it, epn = eps / negative_sample_rate; state next = eps, nneg = epn.
 *     Epoch t = 0 .. n_epochs-1, alpha = 0.25 * (1 - t / n_epochs).  A live arc with next <= t FIRES:
 *       (i)   attraction: D = y_i - Y[j], j = idx_it; d2 and c are part D's; the arc contributes clip(c * D) ONCE (the
 *             target alone moves: there is no factor 2).  next += eps.
 *       (ii)  repulsion: m = trunc((t - nneg) / epn) samples, p = 0 .. m-1.  The hash is part D's with
 *             e = (first_row + i) * k + t_pos (t_pos the arc's list position) and k' = ((z >> 32) * n_ref) >> 32.
 *             D = y_i - Y[k'], the repulsion term is part D's.  No sample is skipped.  nneg += m * epn.
 *       (iii) move: y_i += alpha * S_i.  S_i: lane l of nabo_umap_transform_geometry's `group` lanes takes the list
 *             positions l, l + group, l + 2 group, ... in that order and adds, starting from 0, each arc's contributions
 *             in the order (i) then (ii) p = 0, 1, ...; the lanes' sums are added by TREE (adjacent lanes first).
 *     The reference positions Y are never written.
 *
 * THE DELIBERATE DIFFERENCES from umap-learn 0.5's transform:
 *  1. umap scales eps by the batch's largest membership and floors sigma by the batch's mean distance.  Here the scale is
 *     1 and the floor uses the row's own mean.  A cell's result is then a function of its row, its global row number,
 *     the reference and the parameters only: any split into batches or devices gives the same bits.
 *  2. Epochs are synchronous and seeded, as in part D of nabo_umap.h: each target's displacement of an epoch is one sum
 *     in a fixed order.
 *  3. umap compares a target's number with a sampled reference number and skips the sample on equality, although the
 *     two count different sets of cells.  That comparison is dropped.
 */
#ifndef NABO_UMAP_TRANSFORM_H
#define NABO_UMAP_TRANSFORM_H

#include <stdint.h>

#include "nabo_knn.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nabo_umap_transform nabo_umap_transform;

/* 2 <= n_ref < 2^31, dims 2 or 3.  The parameters start as n_epochs = 100, negative_sample_rate = 5,
 * repulsion_strength = 1, a = 1.577, b = 0.895, seed = 0; the reference positions as zeros; no cells, no batch. */
int nabo_umap_transform_create(nabo_umap_transform **out, int32_t device, int64_t n_ref, int32_t dims);
void nabo_umap_transform_destroy(nabo_umap_transform *T);

/* n_epochs >= 1, negative_sample_rate >= 1, the rest finite, a > 0 and b > 0; else NABO_E_INVALID.  The schedule of a
 * loaded batch is rewound to epoch 0 (which arcs are live depends on n_epochs); its memberships and positions stay. */
int nabo_umap_transform_set_params(nabo_umap_transform *T, int64_t n_epochs, int32_t negative_sample_rate,
                                   double repulsion_strength, double a, double b, uint64_t seed);

/* Y: [n_ref][dims], every value finite: the fitted reference embedding. */
int nabo_umap_transform_set_embedding(nabo_umap_transform *T, const double *Y);

/* The reference cells X [n_ref][g] for nabo_umap_transform_query: a resident k-NN index that is kept for as many
 * batches as follow.  metric and dist_factor are forwarded to the index unchanged. */
int nabo_umap_transform_set_cells(nabo_umap_transform *T, const double *X, int32_t g, int32_t metric, double dist_factor);

/* One batch from its cells Z [m][g] (g as in set_cells): part A' on the resident index -- the lists never visit the
 * host -- then B', C' and the start.  m >= 1, first_row >= 0, (first_row + m) * k < 2^63.  The schedule starts at epoch 0
 * and the positions at the start.  NABO_E_INVALID before nabo_umap_transform_set_cells. */
int nabo_umap_transform_query(nabo_umap_transform *T, int64_t m, int64_t first_row, const double *Z, int32_t k);

/* The same from given lists idx, dist [m][k]: every idx in [0, n_ref), every dist finite and not negative, rows
 * ascending (checked, as nabo_umap_set_knn checks). */
int nabo_umap_transform_set_knn(nabo_umap_transform *T, int64_t m, int64_t first_row, const int64_t *idx, const double *dist,
                                int32_t k);

/* For the tests: memberships memb [m][k] in place of B' and C', every value finite and in [0, 1], every idx in
 * [0, n_ref).  sigma reads back as zeros; the start is that of these memberships (a row whose memberships are all 0
 * has none: set its position). */
int nabo_umap_transform_set_graph(nabo_umap_transform *T, int64_t m, int64_t first_row, const int64_t *idx, const double *memb,
                                  int32_t k);

/* For the tests, of the loaded batch: sigma [m], memb [m][k], the start y0 [m][dims]; any pointer may be NULL.
 * NABO_E_INVALID without a batch. */
int nabo_umap_transform_get_graph(nabo_umap_transform *T, double *sigma, double *memb, double *y0);

/* The batch's positions y: [m][dims], every value finite. */
int nabo_umap_transform_set_positions(nabo_umap_transform *T, const double *y);
int nabo_umap_transform_get_positions(nabo_umap_transform *T, double *y);

/* The next n_run epochs of the batch, from the epoch the last run or rewind left, in ONE launch; never past n_epochs.
 * *done (may be NULL): the epochs run.  The positions and the schedule are written back, so a later run continues:
 * run(p) then run(q) gives the bits of run(p + q). */
int nabo_umap_transform_run(nabo_umap_transform *T, int64_t n_run, int64_t *done);
/* Back to epoch 0 with the schedule's first state; the positions stay. */
int nabo_umap_transform_rewind(nabo_umap_transform *T);

/* For the tests, over the epochs of the last run: per target the attractive terms, the negative samples drawn and the
 * sum (mod 2^64) of the sampled k', [m] each; any may be NULL.  NABO_E_INVALID before the first run of a batch. */
int nabo_umap_transform_last_run_counts(nabo_umap_transform *T, int64_t *n_attr, int64_t *n_neg, uint64_t *idx_sum);

/* Device ms between HIP events: ms[0] the last batch's graph build (B', C', start), ms[1] the k-NN of the last
 * nabo_umap_transform_query (0 after set_knn and set_graph), ms[2] the last run. */
int nabo_umap_transform_last_ms(nabo_umap_transform *T, double ms[3]);

/* How the optimise kernel is built: `group` lanes share one target's list (part D' (iii)).  Needs no device. */
int nabo_umap_transform_geometry(int32_t *group);

#ifdef __cplusplus
}
#endif

#endif /* NABO_UMAP_TRANSFORM_H */
