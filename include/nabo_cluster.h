/*
 * nabo_cluster.h -- C ABI of target classification and of the rings around node sets in libnabo_knn.so (MI355X,
 * gfx950).
 *
 * Replaces two loops of the reference's Graph API (nabo/_graph.py):
 *   classify_target        (:722-792)  per target node, the weight its edges put into every cluster of reference
 *                                      nodes; the node takes the best cluster when that holds more than a fraction
 *                                      of the node's total weight;
 *   get_k_path_neighbours  (:956-987)  the reference nodes at 1, 2, ... hops from a node set (set_de_groups' "Control"
 *                                      cells, :989-1055), read off the hop level of every node.
 * Same conventions as nabo_knn.h: 0 or a negative NABO_E_* status, the message in nabo_last_error(), no CPU fallback
 * (NABO_E_NODEVICE without a device).  Every pointer is a host pointer.
 */
#ifndef NABO_CLUSTER_H
#define NABO_CLUSTER_H

#include <stdint.h>

#include "nabo_graph.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Rows: target node t has the edges nbr[ptr[t] .. ptr[t+1]) with weights w[...], in file order (ptr[0] = 0, monotone,
 * every nbr in [0, n_ref), n_ref < 2^31, at most 4096 edges per row: NABO_E_UNSUPPORTED beyond, one lane walks a
 * row with O(len^2) reads).  A neighbour repeated in a row is ONE edge, at its first position, carrying
 * its LAST weight (what nx.Graph.add_edge does).  ref_cluster[r] is in [0, n_clusters) or -1 (r has no cluster);
 * n_clusters >= 1.  Per target node:
 *   degree = number of distinct neighbours; degree < min_degree: not classified (best / total are still reported);
 *   total  = float64 sum of all merged edge weights in row order, starting from 0;
 *   per cluster, the float64 sum in row order of the weights w > min_weight (strict) whose neighbour has a cluster;
 *   best   = the largest cluster sum (a cluster without such an edge holds 0), ties to the LOWEST cluster id;
 *   label  = the best cluster iff best > weight_frac * total (strict; one float64 product, not fused), else -1.
 * out_label [n_targets]; out_best, out_total: NULL or [n_targets]; out_counts: NULL or [n_clusters + 1], target nodes
 * per label, the last entry counting label -1. */
int nabo_classify_targets(int32_t device, int64_t n_ref, const int32_t *ref_cluster, int32_t n_clusters,
                          int64_t n_targets, const int64_t *ptr, const int64_t *nbr, const double *w,
                          double weight_frac, int64_t min_degree, double min_weight, int32_t *out_label,
                          double *out_best, double *out_total, int64_t *out_counts);

/* Hop levels around node sets on a resident graph.  Set s is members[set_ptr[s] .. set_ptr[s+1]) (set_ptr[0] = 0,
 * monotone; repeats allowed, an empty set allowed; every member in [0, n_nodes)).
 *   out_level[s * n_nodes + v] = hops from v to the nearest member of set s; -1 if unreachable or beyond max_level
 *   (max_level < 0: no limit).
 * 64 sets share one sweep of the graph; the result does not depend on the graph's options or on how the sets fall
 * into sweeps.  nabo_refgraph_last_stats keeps describing the last nabo_refgraph_group_hops call. */
int nabo_refgraph_set_levels(nabo_refgraph *g, int64_t n_sets, const int64_t *set_ptr, const int64_t *members,
                             int32_t max_level, int32_t *out_level);

/* The benchmark's timer (tools/bench_classify.py).  Device time in ms, between HIP events, of the calling thread's last
 * nabo_classify_targets -- ms[0]: the row kernel AND, when out_counts is given, the counts' memset and histogram
 * kernel; uploads and downloads left out -- and last nabo_refgraph_set_levels -- ms[1]: its sweeps from seeding to
 * clearing, per-level host round trips included; the prefill and the download of the levels left out. */
int nabo_cluster_last_device_ms(double ms[2]);

#ifdef __cplusplus
}
#endif

#endif /* NABO_CLUSTER_H */
