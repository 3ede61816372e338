/*
 * nabo_render.h -- C ABI of the rasteriser in libnabo_knn.so (MI355X, gfx950): the laid-out reference graph's nodes and
 * edges aggregated into integer images on the device and composed to one uint8 [H][W][4] picture.
 *
 * Replaces the drawing of GraphPlot (nabo/_graphplot.py:192-274, 434-456): a matplotlib LineCollection / ax.plot of every
 * edge and a scatter of every node, which does not come back for a million nodes and eight million polylines.  Text
 * (labels, title, legend) stays with matplotlib, drawn on top of the image.  Same conventions as nabo_knn.h: 0 or a
 * negative NABO_E_* status, the message in nabo_last_error(), no CPU fallback (NABO_E_NODEVICE without a device).  Every
 * pointer is a host pointer.
 *
 * THE DEFINITION.  The coordinate-to-pixel step is float64, every operation one IEEE - / * floor, never contracted;
 * everything after it is integer arithmetic.  Integer sums: any order of the edges and of the nodes gives the same bits.
 * Canvas: W x H pixels, 1 <= W, H <= 8192, and a viewport (x0, x1, y0, y1) in layout coordinates, finite, x0 < x1, y0 < y1,
 *   x1 - x0 and y1 - y0 finite.
 * Pixel coordinate of a point (x, y):  px = ((x - x0) / (x1 - x0)) * W, then px = min(max(px, -2^20), 2^20); py likewise
 *   with y0, y1, H.  Column u = (int)floor(px), row v = (int)floor(py).  Row 0 is the lowest y:
 *   imshow(img, origin="lower", extent=viewport).
 * Edge layer: one uint32 count per pixel.  Input: E >= 0 polylines, offsets [E+1] with offsets[0] = 0 and at least 2 points
 *   each, every coordinate finite.  A straight edge is a two-point polyline.  Every point goes to its pixel (u, v), which may
 *   lie outside the canvas.  Segment (u0, v0) -> (u1, v1): du = u1 - u0, dv = v1 - v0, s = max(|du|, |dv|); its pixel i is
 *     (u0 + floor((2 * i * du + s) / (2 * s)), v0 + floor((2 * i * dv + s) / (2 * s)))
 *   with floor division of signed 64-bit integers.  A segment draws i = 0 .. s - 1 (nothing if s = 0); after its last
 *   segment a polyline draws its last point's pixel once.  A drawn pixel inside the canvas adds 1, one outside adds nothing.
 *   The rule visits s + 1 distinct, 8-connected pixels and ends exactly on both end pixels (along the longer axis the step is
 *   i itself), so a pixel is hit at most once per segment.  Count a segment with its first point and the closing pixel
 *   with the last point: one pixel then gains at most 1 per point added, and no count can pass 2^32 - 1 while the points
 *   added since the last clear do not.  add_polylines, add_edges and add_bundle return NABO_E_INVALID, and draw nothing,
 *   when the points added since the last clear would exceed 2^32 - 1.
 * Node layer: four uint32 images, count and the sums of R, G and B.  A node has a position, a colour of three uint8 and a
 *   radius R in 1/16 pixel, an integer in 0 .. R_MAX = 1024 (64 pixels; the host converts a radius of r pixels as
 *   floor(r * 16 + 0.5)).  Its centre is (cx, cy) = ((int)floor(px * 16), (int)floor(py * 16)), px and py as above (clamped).
 *   It covers pixel (u, v) iff (16u + 8 - cx)^2 + (16v + 8 - cy)^2 <= R^2, and it always covers the pixel (cx >> 4, cy >> 4)
 *   (arithmetic shift: floor).  A covered pixel inside the canvas adds 1 and the three colour bytes.  255 * count < 2^32
 *   must hold: add_nodes returns NABO_E_INVALID, and draws nothing, when the nodes added since the last clear would
 *   exceed 2^24.
 * Alpha tables: made ON THE HOST by nabo_render_alpha_lut, which the library's own callers use too, so that no pow enters
 *   twice: k = 1 - alpha; t_0 = 1, t_c = t_{c-1} * k; lut[c] = (uint8)floor(255 * (1 - t_c) + 0.5), c = 0 .. L - 1;
 *   2 <= L <= 65536, 0 <= alpha <= 1.  The order-free form of painting c translucent strokes over each other.
 * Compose, per pixel, integers only (/ truncates; every operand is non-negative), with ce the edge count, cn the node
 *   count, (Ce_r, Ce_g, Ce_b) the one edge colour:
 *     Ae = lut_e[min(ce, Le - 1)], An = lut_n[min(cn, Ln - 1)];  Cn_k = (sum_k + cn / 2) / cn, 0 if cn = 0;
 *     t = Ae * (255 - An), den = 255 * An + t;  A = (den + 127) / 255;
 *     C_k = (255 * An * Cn_k + t * Ce_k + den / 2) / den, 0 if den = 0.
 *   Output (C_r, C_g, C_b, A), not premultiplied: nodes lie over edges, the background is transparent.
 * Departures from matplotlib: a pixel's node colour is the MEAN of the nodes covering it, not the last painted, so v_zorder
 *   has no meaning; lines are one pixel wide and not anti-aliased; elw, vlw and vec are accepted by the Python layer and
 *   ignored.  Discs are not anti-aliased either.
 */
#ifndef NABO_RENDER_H
#define NABO_RENDER_H

#include <stdint.h>

#include "nabo_bundle.h"
#include "nabo_knn.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nabo_canvas nabo_canvas;

/* A cleared canvas on `device`.  NABO_E_INVALID unless 1 <= W, H <= 8192 and the viewport is as the definition asks. */
int nabo_render_create(nabo_canvas **out, int32_t device, int32_t W, int32_t H, double x0, double x1, double y0, double y1);
void nabo_render_destroy(nabo_canvas *C);

/* Every image back to 0, the counts of points and nodes added too; the timer starts again with this clear. */
int nabo_render_clear(nabo_canvas *C);

/* "chunk_points": the points (and nodes) staged on the device at a time (1 .. 2^28; results do not depend on it). */
int nabo_render_set_option(nabo_canvas *C, const char *name, int64_t value);

/* offsets: int64 [n_lines + 1]; points: float64 [offsets[n_lines]][2], in layout coordinates.  n_lines = 0 draws nothing. */
int nabo_render_add_polylines(nabo_canvas *C, int64_t n_lines, const int64_t *offsets, const double *points);

/* The straight edges (src[e], dst[e]) of n nodes at (x, y): two-point polylines.  src, dst in [0, n). */
int nabo_render_add_edges(nabo_canvas *C, int64_t n, const double *x, const double *y, int64_t n_edges, const int64_t *src,
                          const int64_t *dst);

/* The polylines a bundle holds, read from its device state (it must live on the canvas's device) and de-normalised by
 * the expression of nabo_bundle_result, c = q * (max - min) + min: the same bits as
 * nabo_render_add_polylines(nabo_bundle_result(B)), without the points visiting the host. */
int nabo_render_add_bundle(nabo_canvas *C, nabo_bundle *B);

/* x, y: [n], finite; radius: [n], in 1/16 pixel, at most R_MAX; rgb: uint8 [n][3]. */
int nabo_render_add_nodes(nabo_canvas *C, int64_t n, const double *x, const double *y, const uint16_t *radius, const uint8_t *rgb);

/* Downloads, uint32 [H][W] each (sums: [H][W][3]); any pointer may be NULL. */
int nabo_render_edge_counts(nabo_canvas *C, uint32_t *counts);
int nabo_render_node_counts(nabo_canvas *C, uint32_t *counts);
int nabo_render_node_sums(nabo_canvas *C, uint32_t *sums);

/* edge_rgb: three bytes; lut_e [Le], lut_n [Ln], 2 <= Le, Ln <= 65536 (nabo_render_alpha_lut); out: uint8 [H][W][4]. */
int nabo_render_compose(nabo_canvas *C, const uint8_t *edge_rgb, const uint8_t *lut_e, int32_t Le, const uint8_t *lut_n, int32_t Ln,
                        uint8_t *out);

/* Device ms since the last clear spent in clear, edges, nodes and compose, and ms[4] their sum (tools/bench_render.py). */
int nabo_render_last_ms(nabo_canvas *C, double ms[5]);

/* The alpha table of the definition.  Needs no device. */
int nabo_render_alpha_lut(double alpha, int32_t L, uint8_t *lut);

/* How the kernels are built: the sub-pixel bits of a node's centre and radius (4), R_MAX, and where the kernels change
 * path -- a segment (after clipping) of up to edge_short_steps pixels is drawn by edge_group lanes, a longer one by a whole
 * wave; a node of radius up to node_small_r (1/16 pixel) by node_group lanes, a larger one by a workgroup.  Any pointer may
 * be NULL.  Needs no device. */
int nabo_render_geometry(int32_t *subpixel_bits, int32_t *r_max, int32_t *edge_short_steps, int32_t *edge_group,
                         int32_t *node_small_r, int32_t *node_group);

#ifdef __cplusplus
}
#endif

#endif /* NABO_RENDER_H */
