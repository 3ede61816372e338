/*
 * nabo_graph.h -- C ABI of the reference-graph path queries in libnabo_knn.so (MI355X, gfx950).
 *
 * Replaces the networkx shortest-path calls of the reference's Graph API (nabo/_graph.py):
 *   get_mapping_specificity (:794-824)  mean hop distance over all pairs of the reference nodes one target node
 *                                       is connected to -- one group per target node;
 *   calc_contiguous_spl     (:904-916)  the same quantity for consecutive nodes of a list -- n-1 two-member groups.
 * Distances are unweighted hop counts on the undirected reference graph.  Same conventions as nabo_knn.h: 0 or a
 * negative NABO_E_* status, the message in nabo_last_error(), no CPU fallback (NABO_E_NODEVICE without a device).
 */
#ifndef NABO_GRAPH_H
#define NABO_GRAPH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nabo_refgraph nabo_refgraph;

/* Upload a graph and keep it resident on `device`.  ptr [n_nodes + 1], nbr [ptr[n_nodes]]: a host CSR whose rows
 * may list arcs in either direction, duplicates and self-loops included; the device copy is the undirected simple
 * graph nx.Graph.add_edge would build (both directions, duplicates merged).  Requires ptr[0] = 0, ptr monotone,
 * every nbr in [0, n_nodes), n_nodes < 2^31 and fewer than 2^30 arcs. */
int nabo_refgraph_create(nabo_refgraph **out, int32_t device, int64_t n_nodes, const int64_t *ptr, const int64_t *nbr);
int nabo_refgraph_destroy(nabo_refgraph *g);

/* Options (the outputs are the same bits whatever their values):
 *   "local_capacity"     nodes a group's search may hold in the local tier's table, 0..896 (default 768;
 *                        0 sends every group to the global tier);
 *   "local_max_members"  largest group the local tier takes, 2..64 (default 64). */
int nabo_refgraph_set_option(nabo_refgraph *g, const char *name, int64_t value);

/* Groups of member nodes: group i is members[grp_ptr[i] .. grp_ptr[i+1]) (grp_ptr[0] = 0, monotone; members may
 * repeat, a repeated pair has distance 0).  For every pair i < j of a group's member POSITIONS:
 *   out_sum[g]        int64 sum of the pair distances of reachable pairs,
 *   out_unreached[g]  number of pairs with no path,
 *   out_pair_hops     NULL, or every pair's distance (-1 = unreachable), groups one after the other, each group's
 *                     m(m-1)/2 pairs in (i, j) lexicographic order. */
int nabo_refgraph_group_hops(nabo_refgraph *g, int64_t n_groups, const int64_t *grp_ptr, const int64_t *members,
                             int64_t *out_sum, int64_t *out_unreached, int32_t *out_pair_hops);

/* Of the last nabo_refgraph_group_hops call.  ms: resident-graph build (at create), local tier, global tier, whole
 * call; counters: groups answered by the local tier, groups sent to the global tier, global sweeps, deepest global
 * BFS level. */
int nabo_refgraph_last_stats(const nabo_refgraph *g, double ms[4], int64_t counters[4]);

/* Of the last nabo_refgraph_group_hops call, out[n_groups]: nodes the local tier's table held when it answered the
 * group, -1 for groups it did not answer (fewer than 2 members, handed to the global tier). */
int nabo_refgraph_last_local_nodes(const nabo_refgraph *g, int64_t n_groups, int32_t *out);

#ifdef __cplusplus
}
#endif

#endif /* NABO_GRAPH_H */
