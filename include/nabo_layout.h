/*
 * nabo_layout.h -- C ABI of the reference graph's 2-D layout in libnabo_knn.so (MI355X, gfx950): ForceAtlas2 with the
 * repulsion summed over every pair.
 *
 * Replaces Graph.set_ref_layout (nabo/_graph.py:179-237), which hands refG to fa2.ForceAtlas2 (Gephi's single-threaded
 * ForceAtlas2; Jacomy et al. 2014), a Python double loop with a Barnes-Hut tree (theta = 1.2).  No tree here: every
 * pair is summed, which is the quantity the tree approximates, and the result is deterministic.  The definition below
 * is the specification; fa2's own floating-point results are not pinned.
 * Same conventions as nabo_knn.h: 0 or a negative NABO_E_* status, the message in nabo_last_error(), no CPU fallback
 * (NABO_E_NODEVICE without a device).  Every pointer is a host pointer.
 *
 * THE DEFINITION.  Nodes are 0 .. n-1.  The graph is undirected, simple and weighted: pairs i < j with a float64
 * weight w.  A pair listed more than once keeps its LAST weight (nx add_edge, as in nabo_cluster.h); a self-loop counts
 * towards the degree and exerts no force.  mass[i] = 1 + deg[i], deg[i] the number of distinct neighbours, the node
 * itself included if it has a self-loop.  A node's row lists its neighbours j != i in ascending j.
 * State per node: x, y, dx, dy, float64 (dx = dy = 0 at the start); scalars speed = 1, eff = 1.
 * comp = mean(mass) with outbound_attraction_distribution (oad), else 1.  One iteration:
 *   1. old = (dx, dy).
 *   2. Repulsion.  xf, yf = x, y rounded to float32.  For every j != i, in float32: ddx = xf_i - xf_j, ddy likewise,
 *      d2 = max(fma(ddy, ddy, ddx * ddx), 2^-100), t = mass_j * rcp(d2) (v_rcp_f32, 1 ulp), and the sums
 *      sx_i += ddx * t, sy_i += ddy * t (fused).  Coincident nodes (and j = i) contribute exactly 0 through the clamp,
 *      without a branch.  A node's sum is taken in float32 over each tile of nabo_layout_geometry's j_tile consecutive
 *      j in ascending j, the tile sums are added in float64 in ascending tile order within a split of consecutive
 *      tiles, and the splits are added in ascending order; rep_i = (scaling_ratio * mass_i) * (sx_i, sy_i), float64.
 *   3. Gravity, float64.  r = sqrt(x^2 + y^2); f = 0 if r == 0, else mass * gravity / r, in strong mode
 *      scaling_ratio * mass * gravity; grav_i = -(x * f, y * f).
 *   4. Attraction, float64, per node over its row in row order, starting from 0: for neighbour j with weight w,
 *      e = 1 if edge_weight_influence == 0, w if it is 1, else pow(w, edge_weight_influence) (evaluated once on the host);
 *      f = -comp * e, divided by mass[min(i, j)] with oad (the LOWER-numbered endpoint's mass divides both ends of an
 *      edge, as fa2 does it); attr_i += ((x_i - x_j) * f, (y_i - y_j) * f).
 *      (dx, dy)_i = (rep_i + grav_i) + attr_i.
 *   5. swing_i = mass_i * |old_i - d_i|, tract_i = 0.5 * mass_i * |old_i + d_i| (|.| = sqrt of the sum of two squares);
 *      S = sum of swing_i, T = sum of tract_i: float64, both by ONE reduction tree in the same kernel (per 256 nodes a
 *      binary tree, then the blocks strided over 256 partial sums in ascending order, then the same binary tree), so
 *      that in the first iteration, where old = 0, S == 2 T exactly and step 6's first comparison is false in every run.
 *   6. Speed, on the device.  If S == 0 or T == 0 the run stops: positions stay as they are, dx, dy hold this
 *      iteration's forces, and the iteration does not count as done (the reference raises ZeroDivisionError).  Else
 *      est = 0.05 * sqrt(n); jt = jitter_tolerance * max(sqrt(est), min(10, est * T / (n * n)));
 *      if S / T > 2.0 { if eff > 0.05: eff *= 0.5;  jt = max(jt, jitter_tolerance) }
 *      target = jt * eff * T / S;
 *      if S > jt * T { if eff > 0.05: eff *= 0.7 } else if speed < 1000: eff *= 1.3;
 *      speed += min(target - speed, 0.5 * speed).
 *   7. Move.  f = speed / (1 + sqrt(speed * swing_i)); x += dx * f, y += dy * f.
 * No atomics anywhere: the same inputs give the same bits on every run.  Rescaling the result (subtracting the minimum
 * x and y, nabo/_graph.py:223-227) is left to the caller.
 */
#ifndef NABO_LAYOUT_H
#define NABO_LAYOUT_H

#include <stdint.h>

#include "nabo_knn.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nabo_layout nabo_layout;

/* The graph as compressed rows in either arc direction: row i lists nbr[ptr[i] .. ptr[i+1]) with weights w[...]
 * (ptr[0] = 0, monotone, every nbr in [0, n), every w finite; 1 <= n < 2^24, so that a mass is exact in float32).  It is
 * made simple as defined above, an arc's position in the arrays deciding which weight is the last.  The state starts as
 * x = y = dx = dy = 0, speed = eff = 1, and the parameters as the reference's defaults (oad = 1,
 * edge_weight_influence = 1, jitter_tolerance = 1, scaling_ratio = 1, strong_gravity_mode = 0, gravity = 1). */
int nabo_layout_create(nabo_layout **out, int32_t device, int64_t n, const int64_t *ptr, const int64_t *nbr, const double *w);
void nabo_layout_destroy(nabo_layout *L);

/* All finite, or NABO_E_INVALID.  barnes_hut_theta is accepted and ignored: there is no tree. */
int nabo_layout_set_params(nabo_layout *L, int32_t outbound_attraction_distribution, double edge_weight_influence,
                           double jitter_tolerance, double scaling_ratio, int32_t strong_gravity_mode, double gravity,
                           double barnes_hut_theta);

/* x, y, dx, dy: [n] each.  set: dx and dy may both be NULL (zeros). */
int nabo_layout_set_state(nabo_layout *L, const double *x, const double *y, const double *dx, const double *dy, double speed,
                          double eff);
int nabo_layout_get_state(nabo_layout *L, double *x, double *y, double *dx, double *dy, double *speed, double *eff);

/* Up to n_iter iterations, queued without a host round trip in between; *done (may be NULL) = the iterations that moved
 * the nodes: n_iter, or fewer when step 6 stopped the run. */
int nabo_layout_run(nabo_layout *L, int64_t n_iter, int64_t *done);

/* For the tests: the three parts of (dx, dy) of the last iteration run, [n][2] each (x then y per node), and
 * st = {S, T} of step 5.  Any pointer may be NULL.  NABO_E_INVALID before the first iteration. */
int nabo_layout_last_forces(nabo_layout *L, double *repulsion, double *gravity, double *attraction, double st[2]);

/* The benchmark's timer (tools/bench_layout.py).  Device time in ms between HIP events of the last nabo_layout_run:
 * ms[0..4] the pack, repulsion, node, speed and move kernels, each the MEAN per iteration over the run's last *n_timed
 * iterations (at most 16 are timed); ms[5] the whole run, from its first launch to its last. */
int nabo_layout_last_ms(nabo_layout *L, double ms[6], int64_t *n_timed);

/* How the repulsion kernel is built: i_block nodes per workgroup, j_tile nodes per staged tile, and for a graph of n
 * nodes the number of splits the tiles are summed in.  Needs no device. */
int nabo_layout_geometry(int64_t n, int32_t *i_block, int32_t *j_tile, int32_t *n_splits);

#ifdef __cplusplus
}
#endif

#endif /* NABO_LAYOUT_H */
