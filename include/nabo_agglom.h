/*
 * nabo_agglom.h -- C ABI of the greedy modularity agglomeration of the reference graph in libnabo_knn.so (MI355X,
 * gfx950): n clusters for any n, and the whole hierarchy they are read from.  It works on the handle of
 * nabo_community.h and extends that header; it is a file of its own because the entry points of nabo_community.h are
 * counted by that header's checks.
 *
 * Replaces Graph.make_clusters (nabo/_graph.py:247-264: Newman's 2004 greedy agglomeration through the `hac` package,
 * the dendrogram kept in `_agglomDendrogram`).  Newman's algorithm takes one merge at a time; the definition below takes a
 * greedy matching per round and is the specification; hac's own merge order is not pinned.  Same
 * conventions as nabo_community.h: 0 or a negative NABO_E_* status, the message in nabo_last_error(), no CPU fallback,
 * every pointer a host pointer.
 *
 * THE DEFINITION.  Graph, quantising, k, in and 2m are those of nabo_community.h.  The modularity is at resolution 1, as
 * Newman's and hac's is.  A run starts at level 0 with every node a cluster of its own.
 *
 * Gain.  For two clusters c != d of the current level joined by an arc of weight a_cd, D(c, d) = a_cd * 2m - k_c * k_d, a
 * signed 128-bit integer, |D| < 2^106.  Merging them changes Q by exactly 2 D / (2m)^2.  Only pairs with an arc can merge.
 *
 * Pair order.  Pairs {c, d} with c < d are ordered by D descending, then c ascending, then d ascending: a strict total
 * order.
 *
 * Round.  The round's matching is the greedy matching of the pairs with D > 0 in pair order: go through them and take a
 * pair if both its ends are still free.  If there is no pair with D > 0 but there is an arc, the round takes the single
 * first pair of the order.  If there is no arc, the run ends.  The taken pairs, in pair order, are appended to the
 * dendrogram; if taking all of them would leave fewer than n_min clusters, only the first (clusters - n_min) are taken and
 * the run ends.  Then comm[d] = c for every taken pair (the lower id survives), comm[i] = i otherwise, and the
 * aggregation of nabo_community.h makes the next level.  Ids are renumbered in ascending old id, so the id order of the
 * clusters is always the order of their smallest level-0 members; that member is the cluster's representative, rep.
 *
 * How the device computes the matching: locally dominant passes.  In a pass every free cluster c picks, among its free
 * neighbours d with D(c, d) > 0, the pair {c, d} that is first in pair order; c and d are matched iff they picked each
 * other.  Passes repeat until a pass matches nothing; `passes` counts the passes run, that last one included.  Because
 * the order is strict and both ends of a pair see it alike, the first pair of the order among the free clusters is
 * always mutual, so every pass with a candidate matches at least one pair, and the pairs matched are exactly those of the
 * greedy matching (DESIGN.md 4.18 has the argument).  The round without a positive gain finds its one pair by one pass
 * more over the gains of every sign, which is not counted.
 *
 * Dendrogram.  One record per merge, in order: rep_a < rep_b, round, a_cd, k_a, k_b, all int64.  The running exact sums
 * follow from them: sum_in += 2 a_cd, sum_d2 += 2 k_a k_b, starting at the singletons' sum of in_i and sum of k_i^2.
 * q_path[t], the Q after t merges, is the modularity of nabo_community.h from these sums at resolution 1;
 * X_t = sum_in * 2m - sum_d2 is the exact integer Q (2m)^2.
 *
 * Cut.  cut(n_clusters) applies the first n0 - n_clusters merges; n_clusters = 0 means the peak, the earliest t that
 * maximises X_t.  NABO_E_INVALID if n_clusters lies outside [the clusters at the end of the run, n0].  Labels are 1 .. C
 * by descending node count, ties by smallest member: the numbering of nabo_community_split with split = 0.  Clusters are
 * connected by construction, so there is no split step.  Every quantity is an exact integer or comes from one: the same
 * call gives the same bytes every time.
 */
#ifndef NABO_AGGLOM_H
#define NABO_AGGLOM_H

#include "nabo_community.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The whole run from level 0 until n_min clusters are left (1 <= n_min <= n, else NABO_E_INVALID) or no arc is; it leaves
 * the handle at the last level reached and keeps the dendrogram until the next run. */
int nabo_community_agglomerate(nabo_community *H, int64_t n_min);
/* Of the last run: *n_merges first (the arrays may be NULL), then up to `cap` records as int64 [cap][6] and the Q after
 * 0 .. min(cap, *n_merges) merges in q_path [cap + 1]. */
int nabo_community_dendrogram(nabo_community *H, int64_t *n_merges, int64_t cap, int64_t *rec, double *q_path);
/* Of the last run: info[0] the rounds, info[1] the passes, info[2] the number of merges at the peak, info[3] the clusters
 * at the end of the run. */
int nabo_community_agglom_info(nabo_community *H, int64_t info[4]);
/* The partition after n0 - n_clusters merges of the last run (n_clusters = 0: the peak): labels [n] in 1 .. *n_out, *q its
 * modularity.  Any pointer may be NULL. */
int nabo_community_cut(nabo_community *H, int64_t n_clusters, int32_t *labels, int32_t *n_out, double *q);

/* For the tests: one pass on the current level.  free [n], 0 = not free (NULL: every cluster is free); partner [n], -1
 * for none; the winning D as d_hi (the high 64 bits, signed) and d_lo (the low 64), 0 for none. */
int nabo_community_match_pass(nabo_community *H, const uint8_t *free, int32_t *partner, int64_t *d_hi, uint64_t *d_lo);
/* For the tests: one round's matching on the current level.  pairs: int32 [n / 2][2], the pairs (c < d) in pair order
 * (may be NULL).  It leaves comm set for all of them, so that nabo_community_aggregate follows. */
int nabo_community_match(nabo_community *H, int64_t *n_pairs, int64_t *passes, int32_t *pairs);

/* The benchmark's timer (tools/bench_agglom.py), device ms between HIP events of the last run: ms[0] the passes, ms[1]
 * the ordering of the pairs, ms[2] the aggregations, ms[3] the whole run. */
int nabo_community_agglom_ms(nabo_community *H, double ms[4]);

#ifdef __cplusplus
}
#endif

#endif /* NABO_AGGLOM_H */
