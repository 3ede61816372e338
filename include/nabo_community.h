/*
 * nabo_community.h -- C ABI of the clustering of the reference graph in libnabo_knn.so (MI355X, gfx950): seeded
 * synchronous Louvain on exact integers, a split into connected components, and the modularity of any labelling.
 *
 * Replaces Graph.make_leiden_clusters (nabo/_graph.py:266-292: leidenalg + igraph on refG, RB configuration model,
 * `resolution`, `random_seed`) and Graph.calc_modularity (:415-442).  The definition below is the specification;
 * leidenalg's own partitions and its random stream are not pinned.  Same conventions as nabo_layout.h:
 * 0 or a negative NABO_E_* status, the message in nabo_last_error(), no CPU fallback (NABO_E_NODEVICE without a
 * device).  Every pointer is a host pointer.
 *
 * THE DEFINITION.  Nodes are 0 .. n-1.
 *
 * Graph.  The input is a CSR (ptr, nbr, w) in either arc direction, made simple exactly as nabo_layout.h does it: a
 * pair listed more than once keeps its LAST weight (an arc's position in the arrays decides), self-loops are kept.
 *
 * Quantising.  q = rint(w * weight_scale) (float64 product, round half to even).  Nabo's SNN weights are hundredths
 * (nabo/_mapping.py:194), so with weight_scale = 10000 they quantise exactly.  Pairs with q == 0 are dropped, their
 * nodes stay.  NABO_E_INVALID for a negative or non-finite weight, for q > 2^31, or if 2m >= 2^53.
 *
 * Per node i, all exact int64: a_ij the off-diagonal weights, s_i the self-loop weight, k_i = sum_j a_ij + 2 s_i the
 * degree, in_i = s_i the inner weight; 2m = sum_i k_i.  (As the reference's calc_modularity: a self-loop counts twice
 * in the degree and once inside its community.)
 *
 * Level.  A level is (n, a, k, in); comm[i] = i at the start of a level.  Per community c, recomputed from comm at each
 * sweep start: tot[c] = sum of k_i over i in c, size[c] = the number of members.
 *
 * One sweep (level L, sweep s, resolution g) is SYNCHRONOUS: every read is of the state at sweep start.  For node i in
 * community a:
 *   1. t_i = (g * (double)k_i) / (double)2m.
 *   2. The candidates are the communities of its neighbours j != i, plus a.  Each candidate C has the exact integer
 *      e_iC = sum of a_ij over j in C, j != i (0 for a if no neighbour is in a).
 *   3. T_C = tot[C], except T_a = tot[a] - k_i.
 *   4. score(C) = (double)e_iC - t_i * (double)T_C: the multiply and the subtract each rounded once, no fma.  All
 *      integers are below 2^53, so the conversions are exact.
 *   5. best = the candidate of largest score, the LOWEST community id on ties.
 *   6. i WANTS to move iff it has at least one neighbour j != i, best != a, score(best) > score(a) strictly, and NOT
 *      (size[a] == 1 && size[best] == 1 && best > a) -- the singleton-swap rule of Lu, Halappanavar & Kalyanaraman 2015.
 *   7. i is ACTIVE iff the top bit of mix(mix(mix(seed + G (L + 1)) + G (s + 1)) + G (i + 1)) is set; mix and G are
 *      those of nabo_umap.h, in wrapping unsigned 64-bit arithmetic.
 *   8. i moves to best iff it wants to and is active.
 * The sweep reports `want` and `moved`, the numbers of such nodes.  (Without the gate the synchronous sweep oscillates.)
 *
 * Phase.  Sweeps s = 0, 1, ... until a sweep reports want == 0 or max_sweeps sweeps have run.  `sweeps` counts the
 * sweeps run, the one that reported want == 0 included.
 *
 * Aggregation.  If the phase moved no node at all, the run ends.  Otherwise the used community ids are renumbered
 * 0 .. n'-1 in ascending old id; a'_cd = sum of a_ij over i in c, j in d, for c != d; k'_c = sum of k_i;
 * in'_c = sum of in_i + sum of a_ij over i, j in c, i != j (each pair is seen from both ends: an inner edge adds 2 a).
 * The run goes on at level L + 1, up to max_levels levels.
 *
 * Modularity of a partition, on the host from exact integers:
 *   Q = (double)(sum_c in_c) / (double)2m - g * ((double)(sum_c d_c^2) / ((double)2m * (double)2m)),
 * d_c the sum of its members' degrees, sum d_c^2 taken in an unsigned 128-bit integer (it is <= (2m)^2 < 2^106), each
 * conversion rounding to nearest, nothing fused.  With g = 1 this is what Graph.calc_modularity computes.  Q = 0 if
 * 2m == 0.
 *
 * Result.  Among the singleton partition and the partition after each level, the one of largest Q, the earliest on
 * ties.  With `split`, each of its communities is replaced by the connected components it has in the level-0 graph
 * (arcs a_ij > 0 between members): Leiden's guarantee; it never lowers Q for g >= 0 (in is unchanged, sum d^2 shrinks).
 * Final labels are 1 .. C by descending node count, ties by smallest member id (leidenalg's numbering + 1, as the
 * reference stores it).  The Q of the final labels and the history are kept: one record (n, n', sweeps, moved, Q) per
 * phase run, Q that of the partition after the level; the phase that moved nothing, if the run ended by one, is
 * recorded too, with n' = n.
 *
 * Every accumulation is an integer one, so any order of summation gives the same bits, and nothing depends on the
 * order of arrival: the same call gives the same labels on every run.
 */
#ifndef NABO_COMMUNITY_H
#define NABO_COMMUNITY_H

#include <stdint.h>

#include "nabo_knn.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nabo_community nabo_community;

/* The graph as nabo_layout_create takes it (ptr[0] = 0, monotone, every nbr in [0, n); 1 <= n < 2^31), quantised with
 * weight_scale (finite, positive).  The parameters start as resolution = 1, seed = 4466, max_sweeps = 128,
 * max_levels = 32, split = 1; the handle stands at level 0 with comm[i] = i. */
int nabo_community_create(nabo_community **out, int32_t device, int64_t n, const int64_t *ptr, const int64_t *nbr, const double *w,
                          double weight_scale);
void nabo_community_destroy(nabo_community *H);

/* resolution finite and >= 0, max_sweeps >= 1, max_levels >= 1; else NABO_E_INVALID. */
int nabo_community_set_params(nabo_community *H, double resolution, uint64_t seed, int32_t max_sweeps, int32_t max_levels,
                              int32_t split);

/* The whole run from level 0; it leaves the handle at the last level reached. */
int nabo_community_run(nabo_community *H);
/* Of the last run: labels [n] in 1 .. *n_clusters, the Q of these labels.  Any pointer may be NULL. */
int nabo_community_labels(nabo_community *H, int32_t *labels, int32_t *n_clusters, double *q);
/* Of the last run: *n_records first (the arrays may be NULL), then up to `cap` records: n, n_next, sweeps, moved as
 * int64 [cap][4], q [cap]. */
int nabo_community_history(nabo_community *H, int64_t *n_records, int64_t cap, int64_t *rec, double *q);

/* The modularity of ANY labelling of the level-0 nodes (labels [n], any int32 values; equal value = same cluster). */
int nabo_community_modularity(nabo_community *H, const int32_t *labels, double resolution, double *q);
/* The result step alone on a labelling of the level-0 nodes: with split != 0 every cluster is replaced by its connected
 * components, then the clusters are numbered 1 .. *n_clusters by size as defined above.  out: [n]. */
int nabo_community_split(nabo_community *H, const int32_t *labels, int32_t split, int32_t *out, int32_t *n_clusters);

/* For the tests: the current level.  n nodes, n_arcs off-diagonal arcs (both directions counted), two_m = 2m. */
int nabo_community_level_size(nabo_community *H, int64_t *n, int64_t *n_arcs, int64_t *two_m);
/* ptr [n + 1], nbr [n_arcs], a [n_arcs], k [n], in [n]; rows in ascending neighbour; any pointer may be NULL. */
int nabo_community_get_level(nabo_community *H, int64_t *ptr, int64_t *nbr, int64_t *a, int64_t *k, int64_t *in);
/* comm [n] of the current level, every entry in [0, n). */
int nabo_community_set_comm(nabo_community *H, const int32_t *comm);
int nabo_community_get_comm(nabo_community *H, int32_t *comm);
/* One sweep of the current level from the current comm, with the gate of (level, sweep). */
int nabo_community_sweep(nabo_community *H, int64_t level, int64_t sweep, int64_t *moved, int64_t *want);
/* Aggregates the current level by its comm; the coarse level becomes the current one, with comm[i] = i. */
int nabo_community_aggregate(nabo_community *H);
/* Back to level 0 with comm[i] = i. */
int nabo_community_rewind(nabo_community *H);

/* The benchmark's timer (tools/bench_community.py), device ms between HIP events of the last run: ms[0] the sweeps,
 * ms[1] the aggregations, ms[2] the split and the final modularity, ms[3] the whole run. */
int nabo_community_last_ms(nabo_community *H, double ms[4]);

/* How the sweep is built: `group` lanes share a row of at most `long_threshold` arcs; a longer row takes a workgroup
 * with a table in LDS that holds `table_capacity` distinct neighbour communities; a row with more takes a table in
 * global memory.  Needs no device. */
int nabo_community_geometry(int32_t *group, int32_t *long_threshold, int32_t *table_capacity);

#ifdef __cplusplus
}
#endif

#endif /* NABO_COMMUNITY_H */
