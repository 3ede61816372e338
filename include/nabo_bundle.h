/*
 * nabo_bundle.h -- C ABI of edge bundling in libnabo_knn.so (MI355X, gfx950): the laid-out reference graph's edges drawn
 * towards each other by advection along the gradient of their own density.
 *
 * Replaces the bundling of GraphPlot(..., bundle_edges=True) (nabo/_graphplot.py:192-220), which hands the node positions
 * and the edge list to datashader.bundling.hammer_bundle: Python and numba on one core over every sample point of every
 * edge.  datashader and skimage are not pinned here; the definition below is the specification, and it says where it
 * departs from datashader.  Same conventions as nabo_knn.h: 0 or a negative NABO_E_* status, the message in
 * nabo_last_error(), no CPU fallback (NABO_E_NODEVICE without a device).  Every pointer is a host pointer.
 *
 * THE DEFINITION.  All arithmetic is float64; every operation is one IEEE + - * / sqrt, never contracted into an fma;
 * every sum runs in the order stated.  (int)(.) truncates.
 * Input: n nodes with finite x, y; E >= 1 edges (src, dst) in caller order, duplicates and self-loops kept as given (a
 * self-loop is a two-point polyline of length 0).  Each coordinate c is normalised to q = (c - min) / (max - min) over the
 * nodes, q = 0 if max == min.  An edge starts as the two points {q[src], q[dst]}.
 * Parameters (datashader's defaults): initial_bandwidth 0.05, decay 0.7, iterations 4, accuracy A = 500 (2 <= A <= 4096),
 * advect_iterations 50, resample_every 2, min_segment_length 0.008, max_segment_length 0.016, tension 0.3,
 * smooth_passes 10; batch_size is accepted and ignored.  P_MAX = 256 points per edge (nabo_bundle_geometry).
 *
 * Resample of one polyline P_0 .. P_{p-1}, tl = (min_segment_length + max_segment_length) / 2:
 *   seg_j = sqrt(dx * dx + dy * dy) of P_{j+1} - P_j;  c_0 = 0, c_{j+1} = c_j + seg_j in ascending j;  L = c_{p-1};
 *   m = clamp(ceil(L / tl) + 1, 2, P_MAX).  If L == 0 the result is {P_0, P_{p-1}}.  Otherwise Q_0 = P_0 and
 *   Q_{m-1} = P_{p-1} are copied, and for 0 < i < m-1:  t = i * (L / (m-1));  j = the largest index with c_j <= t, at most
 *   p-2;  f = (t - c_j) / seg_j, 0 if seg_j == 0;  Q_i = P_j + (P_{j+1} - P_j) * f per coordinate.
 *   The integer decisions are m and every j.  (datashader splits and merges segments against the two limits; this
 *   re-spaces evenly by arc length.)
 * Pixel of a point: u = min(max((int)(qx * A), 0), A), v likewise from qy.
 * Density: an (A+1) x (A+1) image of unsigned 32-bit counts; every point of every edge, end points included, adds 1 at
 *   [u][v].  Integer sums: any order gives the same bits.  No float atomics anywhere.
 * Field for a bandwidth of b pixels: sigma = b / 2, R = ceil(4 * sigma), w_t = exp(-0.5 * (t / sigma)^2) for t = -R .. R,
 *   divided by their sum taken in ascending t -- made ON THE HOST by nabo_bundle_blur_weights, which the library itself
 *   calls, so that no exp enters twice.  The blur is separable, along the first axis and then along the second, zeros
 *   outside the image: per output acc = 0; acc = acc + w_t * v for t = -R .. R ascending (terms outside the image add
 *   exactly 0 and are skipped).  D = B / max(B).  gx[u][v] = D[min(u+1, A)][v] - D[max(u-1, 0)][v], gy likewise along v;
 *   mag = sqrt(gx * gx + gy * gy) + 1e-5; the field is (GX, GY) = (gx / mag, gy / mag).
 *   (datashader takes skimage's Sobel; this is a central difference of an image that is smooth already.)
 * Advection step: every interior point moves to qx = min(max(qx + GX[u][v] / A, 0), 1), qy likewise with GY, (u, v) its
 *   pixel before the move; end points never move.  Within a round of s steps the edge is resampled after every
 *   resample_every-th step and after the last one.
 * Run: resample the straight edges.  d_1 = decay, d_{i+1} = d_i * decay.  For i = 1 .. iterations:
 *   b = (initial_bandwidth * d_i) * A; stop if b < 2; else density, field(b), one round of advect_iterations steps.
 *   Then smooth_passes synchronous passes: every interior point becomes ((1 - tension) * P_j) + ((tension * 0.5) *
 *   (P_{j-1} + P_{j+1})), all from the previous pass's points (datashader smooths in place).  Then de-normalise:
 *   c = q * (max - min) + min.
 * Output: offsets, int64 [E+1], and points, float64 [offsets[E] + E][2], in input edge order, each edge followed by one
 *   NaN row: ax.plot(pts[:,0], pts[:,1]) draws it.  (The reference drops datashader's NaN rows and so joins consecutive
 *   edges; that is not reproduced.)
 * Edges are coupled only through the field, and an edge's result does not depend on which kernel or group computed it:
 * the same inputs give the same bits on every run, and permuting the edges permutes the polylines.
 */
#ifndef NABO_BUNDLE_H
#define NABO_BUNDLE_H

#include <stdint.h>

#include "nabo_knn.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nabo_bundle nabo_bundle;

/* x, y: [n], finite; src, dst: [n_edges], in [0, n); n >= 1, n_edges >= 1.  The state starts as the straight two-point
 * edges, normalised, and the parameters as the defaults. */
int nabo_bundle_create(nabo_bundle **out, int32_t device, int64_t n, const double *x, const double *y, int64_t n_edges,
                       const int64_t *src, const int64_t *dst);
void nabo_bundle_destroy(nabo_bundle *B);

/* NABO_E_INVALID unless: initial_bandwidth finite and > 0, 0 < decay <= 1, iterations >= 0, 2 <= accuracy <= 4096,
 * advect_iterations >= 0, resample_every >= 1, 0 < min_segment_length <= max_segment_length (finite), 0 <= tension <= 1,
 * smooth_passes >= 0.  batch_size is ignored. */
int nabo_bundle_set_params(nabo_bundle *B, double initial_bandwidth, double decay, int32_t iterations, int32_t accuracy,
                           int32_t advect_iterations, int32_t resample_every, double min_segment_length,
                           double max_segment_length, double tension, int32_t smooth_passes, int64_t batch_size);

/* "chunk_edges": the edges whose result slots are on the device at a time (>= 1; results do not depend on it). */
int nabo_bundle_set_option(nabo_bundle *B, const char *name, int64_t value);

/* The state: offsets [E+1] and the normalised points [offsets[E]][2], edge after edge.  get: either may be NULL
 * (*n_points, if given, is offsets[E]).  set: offsets[0] = 0, every edge 2 .. 2 * P_MAX points (more than a resample ever
 * yields, so that a test can hand over a longer polyline), every coordinate in [0, 1]. */
int nabo_bundle_get_points(nabo_bundle *B, int64_t *n_points, int64_t *offsets, double *points);
int nabo_bundle_set_points(nabo_bundle *B, const int64_t *offsets, const double *points);

/* The single steps of the definition, each on the state as it is. */
int nabo_bundle_resample(nabo_bundle *B);
/* image: [(A+1)][(A+1)] counts (may be NULL: the image stays on the device for nabo_bundle_field) */
int nabo_bundle_density(nabo_bundle *B, uint32_t *image);
/* the field of the last density for a bandwidth of b pixels (0.5 <= b <= 16384); blurred (B, before the division by its
 * maximum), gx, gy (GX, GY): [(A+1)][(A+1)] each, any may be NULL */
int nabo_bundle_field(nabo_bundle *B, double b, double *blurred, double *gx, double *gy);
/* one round of n_steps >= 1 steps along the last field */
int nabo_bundle_advect(nabo_bundle *B, int64_t n_steps);
int nabo_bundle_smooth(nabo_bundle *B, int64_t passes);

/* The whole run from the state as it is (after create: the straight edges), and its de-normalised, NaN-separated result:
 * offsets [E+1], points [offsets[E] + E][2]; either may be NULL. */
int nabo_bundle_run(nabo_bundle *B);
int nabo_bundle_result(nabo_bundle *B, int64_t *offsets, double *points);

/* The benchmark's timer (tools/bench_bundle.py): device ms of the last nabo_bundle_run spent in resample, density, field,
 * advect and smooth, and ms[5] their sum. */
int nabo_bundle_last_ms(nabo_bundle *B, double ms[6]);

/* How the round kernels are built: P_MAX; the lanes that share a short edge and the points such an edge may hold (an
 * edge that outgrows them is redone by a whole wave); the lanes of a long edge.  Needs no device. */
int nabo_bundle_geometry(int32_t *p_max, int32_t *short_group, int32_t *short_cap, int32_t *long_group);

/* *R = ceil(4 * (b / 2)) and, if w is given (cap >= 2 * R + 1 doubles), the normalised weights w[t + R].  Needs no device. */
int nabo_bundle_blur_weights(double b, int32_t *R, double *w, int64_t cap);

#ifdef __cplusplus
}
#endif

#endif /* NABO_BUNDLE_H */
