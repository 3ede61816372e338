/*
 * nabo_umap.h -- C ABI of the UMAP embedding of cells in libnabo_knn.so (MI355X, gfx950): exact k-NN, fuzzy graph,
 * synchronous epochs.
 *
 * Replaces nabo.make_umap (nabo/_umap.py:7-39), which hands the PCA coordinates to umap.UMAP (umap-learn 0.5: NN-descent,
 * numba).  The definition below is the specification; umap-learn's own floating-point results and its random stream
 * are not pinned.  It follows umap-learn part by part; part D is the one deliberate change.
 * Same conventions as nabo_knn.h: 0 or a negative NABO_E_* status, the message in nabo_last_error(), no CPU fallback
 * (NABO_E_NODEVICE without a device).  Every pointer is a host pointer.
 *
 * THE DEFINITION.  Cells are 0 .. n-1, everything is float64 unless said otherwise, no operation is fused.
 *
 * A. Neighbours.  idx[n][k], dist[n][k]: each cell's k = n_neighbors nearest cells, itself included, in (dist asc,
 *    idx asc) order -- what nabo_index_query returns for X against X with drop_first = 0.  2 <= k <= NABO_MAX_K, k < n.
 *    The entries of a row are distinct cells.
 *
 * B. Smooth distances (smooth_knn_dist, local_connectivity = 1, bandwidth = 1).  TREE(v_0 .. v_{k-1}) below is the sum
 *    by a binary tree over W slots, W the smallest power of two >= k, slots >= k holding 0: adjacent slots are added
 *    (0+1, 2+3, ...), then adjacent pair sums, and so on.
 *      rho_i   = the smallest positive entry of row i (the first one, the row ascends), 0 if there is none.
 *      psum(m) = TREE(v), v_0 = 0 and for t = 1 .. k-1: v_t = 1 if d_t - rho_i <= 0, else exp(-((d_t - rho_i) / m)).
 *                Position 0 is skipped whatever it holds, as umap skips it.
 *      sigma_i : target = log2(k) (float64 log2); lo = 0, hi = inf, mid = 1; at most 64 steps of
 *                  p = psum(mid); if |p - target| < 1e-5 stop;
 *                  if p > target { hi = mid; mid = (lo + hi) / 2 }
 *                  else { lo = mid; if hi is infinite mid = mid * 2, else mid = (lo + hi) / 2 }
 *                sigma_i = mid.  lo, hi and mid are dyadic and exact, so sigma has the same bits wherever every
 *                comparison falls the same way.
 *      floor   : rowsum_i = TREE(d_0 .. d_{k-1}).  If rho_i > 0: mean = rowsum_i / k; else mean = total / (n k), where
 *                total adds the rowsum_i into 256 accumulators, accumulator c taking rows c, c + 256, c + 512, ... in
 *                ascending order, and then adds the accumulators by halving (c += c + 128, then + 64, ... + 1).
 *                sigma_i = max(sigma_i, 1e-3 * mean).
 *
 * C. Fuzzy graph.  For row i, position t, j = idx[i][t], d = dist[i][t]:
 *      a_ij = 0 if j == i;  1 if d - rho_i <= 0 or sigma_i == 0;  exp(-((d - rho_i) / sigma_i)) otherwise;
 *      a_ij = 0 for every j that row i does not list.
 *    Union: w_ij = (a_ij + a_ji) - a_ij * a_ji for every pair i != j that either row lists: the same bits from both
 *    ends.  Prune: wmax = the largest w; arcs with w < wmax / n_epochs (n_epochs as float64) are dropped.  The result is
 *    a symmetric CSR: row i holds its arcs (i -> j) in ascending j.  e below is an arc's position in this CSR.
 *
 * D. Epochs -- the deliberate difference.  umap-learn updates positions in place, arc by arc, which under numba's
 *    parallel=True is a data race.  Here an epoch is SYNCHRONOUS: every read is of the positions y at the start of the
 *    epoch, every node's displacement is a sum the node alone owns, positions are double-buffered, and there are no
 *    atomics: the same call gives the same bits on every run.
 *    Per arc e = (i -> j): eps_e = wmax / w_e, epn_e = eps_e / negative_sample_rate; state next_e = eps_e,
 *    nneg_e = epn_e (umap's recurrence, in float64: + - * / and truncation only).
 *    Epoch t = 0 .. n_epochs-1, alpha = 1 - t / n_epochs.  Every arc with next_e <= t FIRES:
 *      (i)   attraction: D = y_i - y_j per component, d2 = sum of D*D in component order;
 *            c = d2 > 0 ? (ca * pow(d2, b - 1)) / (a * pow(d2, b) + 1) : 0, ca = (-2 * a) * b;
 *            g = clip(c * D, -4, 4) per component; the arc contributes 2 * g to node i (the factor 2 is umap's
 *            move_other: the arc (j -> i) has the same weight, hence the same schedule, and its update of i equals g).
 *            next_e += eps_e.
 *      (ii)  repulsion: m = trunc((t - nneg_e) / epn_e) samples, p = 0 .. m-1.  With G = 0x9E3779B97F4A7C15 and
 *            mix(z) = { z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
 *            z ^ (z >> 31) } in wrapping unsigned 64-bit arithmetic:
 *              s_t = mix(seed + G * (t + 1)),  s_e = mix(s_t + G * (e + 1)),  z = mix(s_e + G * (p + 1)),
 *              k' = ((z >> 32) * n) >> 32        (n < 2^31)
 *            k' == i contributes nothing.  Otherwise D = y_i - y_k', d2 as above,
 *            c = d2 > 0 ? cr / ((0.001 + d2) * (a * pow(d2, b) + 1)) : 0, cr = (2 * gamma) * b, gamma the
 *            repulsion_strength; g = clip(c * D, -4, 4); the sample contributes g to node i only.
 *            nneg_e += m * epn_e (m as float64).
 *      (iii) move: y_i += alpha * S_i.  S_i: lane l of nabo_umap_geometry's `group` lanes takes the row's arcs at row
 *            positions l, l + group, l + 2 group, ... in that order and adds, starting from 0, each arc's
 *            contributions in the order (i) then (ii) p = 0, 1, ...; the lanes' sums are added by the binary tree of
 *            B (adjacent lanes first).  Positions, terms and sums are float64; float32 is used nowhere.
 *    clip(v, -4, 4) = v > 4 ? 4 : v < -4 ? -4 : v.
 *
 * E. Start and curve are the caller's (nabo_amd/_umap.py): the start is brought to [0, 10] per dimension, and a, b are
 *    fitted to umap's curve by a small Levenberg-Marquardt.  dims is 2 or 3.
 */
#ifndef NABO_UMAP_H
#define NABO_UMAP_H

#include <stdint.h>

#include "nabo_knn.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nabo_umap nabo_umap;

/* 3 <= n < 2^31, dims 2 or 3.  The parameters start as n_epochs = 200, negative_sample_rate = 5,
 * repulsion_strength = 1, a = 1.577, b = 0.895 (about spread 1, min_dist 0.1), seed = 0; the embedding as zeros. */
int nabo_umap_create(nabo_umap **out, int32_t device, int64_t n, int32_t dims);
void nabo_umap_destroy(nabo_umap *U);

/* n_epochs >= 1, negative_sample_rate >= 1, the rest finite, a > 0 and b > 0; else NABO_E_INVALID.  A graph built for
 * another n_epochs is dropped (the prune depends on it); otherwise the schedule is rewound to epoch 0. */
int nabo_umap_set_params(nabo_umap *U, int64_t n_epochs, int32_t negative_sample_rate, double repulsion_strength, double a,
                         double b, uint64_t seed);

/* Parts B and C on the device from the lists of part A: idx, dist [n][k]; every idx in [0, n), every dist finite and
 * not negative, rows ascending (checked); the entries of a row distinct (not checked).  The schedule starts at epoch 0. */
int nabo_umap_set_knn(nabo_umap *U, const int64_t *idx, const double *dist, int32_t k);

/* The same from the cells X [n][g]: the lists come from a resident k-NN index (nabo_index_query, X against X,
 * drop_first = 0) and never visit the host.  metric and dist_factor are forwarded to the index unchanged. */
int nabo_umap_fit_knn(nabo_umap *U, const double *X, int32_t g, int32_t k, int32_t metric, double dist_factor);

/* For the tests: a finished graph in place of parts B and C -- a CSR as nabo_umap_get_graph returns it (ptr[0] = 0,
 * monotone; every nbr another node in [0, n); every w finite and positive; at least one arc).  Nothing is pruned or
 * sorted; wmax = the largest w; rho and sigma read back as zeros.  The schedule starts at epoch 0. */
int nabo_umap_set_graph(nabo_umap *U, const int64_t *ptr, const int64_t *nbr, const double *w);

/* For the tests: rho, sigma [n]; the pruned CSR: ptr [n + 1], nbr and w [n_arcs].  nabo_umap_graph_size first; any
 * pointer may be NULL.  NABO_E_INVALID without a graph. */
int nabo_umap_graph_size(nabo_umap *U, int64_t *n_arcs, double *wmax);
int nabo_umap_get_graph(nabo_umap *U, double *rho, double *sigma, int64_t *ptr, int64_t *nbr, double *w);

/* y: [n][dims], every value finite. */
int nabo_umap_set_embedding(nabo_umap *U, const double *y);
int nabo_umap_get_embedding(nabo_umap *U, double *y);

/* The next n_run epochs, from the epoch the last run or rewind left, queued on plain stream launches without a host
 * round trip in between; never past n_epochs.  *done (may be NULL): the epochs run. */
int nabo_umap_run(nabo_umap *U, int64_t n_run, int64_t *done);
/* Back to epoch 0 with the schedule's first state; the embedding stays. */
int nabo_umap_rewind(nabo_umap *U);

/* For the tests, of the last epoch run: per node the attractive terms, the negative samples drawn (those that hit the
 * node itself included) and the sum of the sampled k', [n] each; any may be NULL.  They separate a wrong decision from
 * rounding.  NABO_E_INVALID before the first epoch. */
int nabo_umap_last_epoch_counts(nabo_umap *U, int32_t *n_attr, int32_t *n_neg, uint64_t *idx_sum);

/* The benchmark's timer (tools/bench_umap.py), device ms between HIP events: ms[0] the last graph build (parts B and C;
 * with nabo_umap_fit_knn without the k-NN), ms[1] the k-NN of the last nabo_umap_fit_knn (0 after set_knn), ms[2] the
 * epoch kernel, the MEAN over the last run's last *n_timed epochs (at most 16 are timed), ms[3] the whole last run. */
int nabo_umap_last_ms(nabo_umap *U, double ms[4], int64_t *n_timed);

/* How the epoch kernel is built: `group` lanes share one node's row (part D (iii)).  Needs no device. */
int nabo_umap_geometry(int32_t *group);

#ifdef __cplusplus
}
#endif

#endif /* NABO_UMAP_H */
