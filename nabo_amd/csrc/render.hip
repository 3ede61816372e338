// The rasteriser (include/nabo_render.h is the contract and holds the definition; nabo/_graphplot.py's LineCollection and
// scatter are what it replaces): polylines and discs aggregated into integer images by device-scope integer atomics,
// and one kernel that composes the images to RGBA bytes.
//
// Edges.  The unit of work is a POINT of a polyline: a point that is not its polyline's last stands for the segment to
// the next point (pixels i = 0 .. s - 1), the last one for its own pixel.  One byte per point says which; the host makes
// the bytes for polylines it uploads, a small kernel makes them from a resident bundle's offsets.  A kernel therefore never
// looks up an offset, and a chunk of points is any range of them plus the one point after it.
//   short kernel: RND_EDGE_G = 8 lanes per point, 32 points per workgroup.  It turns the two points into pixels, clips the
//     range of i to what can fall inside the canvas, and draws a range of up to RND_EDGE_SHORT = 64 pixels itself,
//     consecutive lanes on consecutive i -- consecutive pixels of a row for a flat segment.  Bundled polylines have
//     segments of 16 - 32 pixels on a 2048-wide canvas, SNN edges on a layout are mostly shorter still.
//   long kernel: one wave per point of the list the short kernel appended the longer ranges to (an integer atomic; the
//     list's order decides nothing, the sums are integers).  Both kernels run the same device functions.
// Clipping: along each axis the pixel of step i is within 1/2 of a0 + i * d / s, so the steps that can land in [0, N) are
//   those with -a0 - 1 < i * d / s < N - a0: two floor divisions give a range that is never too small, and every pixel of
//   it is still tested against the canvas.  A segment with both end pixels inside needs none of this.  A segment at the
//   +-2^20 clamp has up to 2^21 steps and a range of at most about max(W, H) + 2 of them.
// The step along the longer axis is i itself; the other one is one unsigned division, 32-bit while 2 * s * s + s fits.
// Nodes.  RND_NODE_G = 8 lanes per node walk the node's bounding box of pixels, clipped to the canvas, row by row; a node
//   of radius above RND_NODE_SMALL_R = 56/16 pixel (a box of more than 8 x 8 pixels) goes to a list and gets a whole
//   workgroup.  The four sums of a pixel are two 64-bit words, (count | sum R << 32) and (sum G | sum B << 32): no field
//   can carry into its neighbour while 255 * count < 2^32, and a covered pixel costs two atomics, not four.
// No LDS-tiled, privatised accumulation: DESIGN.md 4.20 has the reasoning and the measurement.
// Bounds: every atomic's pixel is tested against [0, W) x [0, H) by the lane that issues it; a point's successor is read
// only if the point is not marked last, and the last point of every upload and of every bundle is marked.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/nabo_render.h"
#include "bundle_view.h"
#include "host_common.h"

#pragma clang fp contract(off)

namespace nabo {

constexpr int RND_SUB_BITS = 4, RND_R_MAX = 1024;
constexpr int RND_EDGE_G = 8, RND_EDGE_SHORT = 64;
constexpr int RND_NODE_G = 8, RND_NODE_SMALL_R = 56;
constexpr int RND_THREADS = 256;
constexpr int RND_LONG_GRID = 2048;
constexpr int RND_MAX_SIDE = 8192, RND_MAX_LUT = 65536;
constexpr double RND_CLAMP = 1048576.0;   // 2^20
constexpr int64_t RND_CHUNK = (int64_t)1 << 22, RND_MAX_CHUNK = (int64_t)1 << 28;
constexpr uint64_t RND_MAX_POINTS = 0xFFFFFFFFull;
constexpr int64_t RND_MAX_NODES = (int64_t)1 << 24;

struct RenderView {
    int W, H;
    double x0, dx, y0, dy;   // dx = x1 - x0, dy = y1 - y0
};

struct RenderPts {
    const double2 *pts;    // point k; pts[k + 1] is read unless last[k]
    const uint8_t *last;   // [n]
    int64_t n;
    int denorm;            // the points are a bundle's: c = q * span + lo
    double lo[2], span[2];
};

struct RenderNodes {
    const double2 *xy;
    const uint16_t *r;
    const uint8_t *rgb;
    int64_t n;
};

struct RenderSeg {
    int u0, v0, du, dv, s;
    int64_t ilo, ihi;   // the steps to draw
};

struct RenderDisc {
    int cx, cy, R, pu, pv;
    int u0, v0, bw, bh;   // the box of pixels to test, inside the canvas
};

__device__ __forceinline__ double render_coord(double c, double c0, double d, double n)
{
    const double p = ((c - c0) / d) * n;
    return fmin(fmax(p, -RND_CLAMP), RND_CLAMP);
}

__device__ __forceinline__ double2 render_point(const RenderPts &P, int64_t k)
{
    double2 q = P.pts[k];
    if (P.denorm) {
        q.x = q.x * P.span[0] + P.lo[0];
        q.y = q.y * P.span[1] + P.lo[1];
    }
    return q;
}

__device__ __forceinline__ int64_t render_fdiv(int64_t a, int64_t b)   // floor(a / b), b > 0
{
    const int64_t q = a / b;
    return q - ((a % b) < 0);
}

// the steps of [lo, hi] that can put a0 + step(i, d, s) into [0, N): never too few
__device__ __forceinline__ void render_clip_axis(int a0, int d, int s, int N, int64_t &lo, int64_t &hi)
{
    if (d == 0) {
        if (a0 < 0 || a0 >= N) hi = lo - 1;
        return;
    }
    int64_t l, h;
    if (d > 0) {
        l = render_fdiv((int64_t)(-1 - a0) * s, d);
        h = render_fdiv((int64_t)(N - a0) * s, d) + 1;
    } else {
        l = render_fdiv((int64_t)(a0 - N) * s, -(int64_t)d);
        h = render_fdiv((int64_t)(a0 + 1) * s, -(int64_t)d) + 1;
    }
    lo = l > lo ? l : lo;
    hi = h < hi ? h : hi;
}

// floor((2 * i * d + s) / (2 * s)), 0 <= i <= s, |d| <= s; for d < 0 it is -floor((2 * i * |d| + s - 1) / (2 * s))
__device__ __forceinline__ int render_step(int64_t i, int d, int s)
{
    const unsigned a = d < 0 ? (unsigned)-d : (unsigned)d;
    unsigned q;
    if (a == (unsigned)s) q = (unsigned)i;   // (s = 0 comes here too, with i = 0)
    else if (s <= 16384) q = (2u * (unsigned)i * a + (unsigned)s - (d < 0)) / (2u * (unsigned)s);
    else q = (unsigned)((2ull * (uint64_t)i * a + (uint64_t)s - (d < 0)) / (2ull * (uint64_t)s));
    return d < 0 ? -(int)q : (int)q;
}

// what point k draws; false if that is nothing
__device__ __forceinline__ bool render_segment(const RenderView &V, const RenderPts &P, int64_t k, RenderSeg &S)
{
    const double Wd = (double)V.W, Hd = (double)V.H;
    const double2 a = render_point(P, k);
    S.u0 = (int)floor(render_coord(a.x, V.x0, V.dx, Wd));
    S.v0 = (int)floor(render_coord(a.y, V.y0, V.dy, Hd));
    const bool in0 = S.u0 >= 0 && S.u0 < V.W && S.v0 >= 0 && S.v0 < V.H;
    S.du = S.dv = S.s = 0;
    S.ilo = S.ihi = 0;
    if (P.last[k]) return in0;
    const double2 b = render_point(P, k + 1);
    const int u1 = (int)floor(render_coord(b.x, V.x0, V.dx, Wd)), v1 = (int)floor(render_coord(b.y, V.y0, V.dy, Hd));
    S.du = u1 - S.u0;
    S.dv = v1 - S.v0;
    S.s = max(abs(S.du), abs(S.dv));
    S.ihi = (int64_t)S.s - 1;
    if (S.s == 0) return false;
    if (!(in0 && u1 >= 0 && u1 < V.W && v1 >= 0 && v1 < V.H)) {
        render_clip_axis(S.u0, S.du, S.s, V.W, S.ilo, S.ihi);
        render_clip_axis(S.v0, S.dv, S.s, V.H, S.ilo, S.ihi);
    }
    return S.ilo <= S.ihi;
}

__device__ __forceinline__ void render_draw(const RenderView &V, const RenderSeg &S, int64_t i, unsigned int *__restrict__ img)
{
    const int u = S.u0 + render_step(i, S.du, S.s), v = S.v0 + render_step(i, S.dv, S.s);
    if (u >= 0 && u < V.W && v >= 0 && v < V.H) atomicAdd(&img[(size_t)v * V.W + u], 1u);
}

__global__ __launch_bounds__(RND_THREADS) void render_edge_short_kernel(RenderView V, RenderPts P, unsigned int *__restrict__ img,
                                                                        uint32_t *__restrict__ list, unsigned int *n_list)
{
    const int lane = threadIdx.x % RND_EDGE_G;
    const int64_t k = (int64_t)blockIdx.x * (RND_THREADS / RND_EDGE_G) + threadIdx.x / RND_EDGE_G;
    if (k >= P.n) return;
    RenderSeg S;
    if (!render_segment(V, P, k, S)) return;
    if (S.ihi - S.ilo >= RND_EDGE_SHORT) {
        if (lane == 0) list[atomicAdd(n_list, 1u)] = (uint32_t)k;
        return;
    }
    for (int64_t i = S.ilo + lane; i <= S.ihi; i += RND_EDGE_G) render_draw(V, S, i, img);
}

__global__ __launch_bounds__(RND_THREADS) void render_edge_long_kernel(RenderView V, RenderPts P, unsigned int *__restrict__ img,
                                                                       const uint32_t *__restrict__ list, const unsigned int *n_list)
{
    const int lane = threadIdx.x % 64;
    const unsigned int n = *n_list;
    for (unsigned int j = blockIdx.x * (RND_THREADS / 64) + threadIdx.x / 64; j < n; j += gridDim.x * (RND_THREADS / 64)) {
        RenderSeg S;
        if (!render_segment(V, P, (int64_t)list[j], S)) continue;
        for (int64_t i = S.ilo + lane; i <= S.ihi; i += 64) render_draw(V, S, i, img);
    }
}

// last[k] = 1 for the last point of every polyline (last is zero on entry)
__global__ __launch_bounds__(RND_THREADS) void render_mark_kernel(const int64_t *__restrict__ off, int64_t E, uint8_t *__restrict__ last)
{
    const int64_t e = (int64_t)blockIdx.x * RND_THREADS + threadIdx.x;
    if (e < E) last[off[e + 1] - 1] = 1;
}

__device__ __forceinline__ bool render_disc(const RenderView &V, const RenderNodes &N, int64_t k, RenderDisc &D)
{
    const double2 c = N.xy[k];
    D.cx = (int)floor(render_coord(c.x, V.x0, V.dx, (double)V.W) * 16.0);
    D.cy = (int)floor(render_coord(c.y, V.y0, V.dy, (double)V.H) * 16.0);
    D.R = N.r[k];
    D.pu = D.cx >> RND_SUB_BITS;
    D.pv = D.cy >> RND_SUB_BITS;
    // 16u + 8 >= cx - R and 16u + 8 <= cx + R, and the centre's pixel whatever R is
    const int u0 = max(min((D.cx - D.R + 7) >> RND_SUB_BITS, D.pu), 0), u1 = min(max((D.cx + D.R - 8) >> RND_SUB_BITS, D.pu), V.W - 1);
    const int v0 = max(min((D.cy - D.R + 7) >> RND_SUB_BITS, D.pv), 0), v1 = min(max((D.cy + D.R - 8) >> RND_SUB_BITS, D.pv), V.H - 1);
    D.u0 = u0;
    D.v0 = v0;
    D.bw = u1 - u0 + 1;
    D.bh = v1 - v0 + 1;
    return D.bw > 0 && D.bh > 0;
}

// cell c of the disc's box, row by row; img: [H * W][2] words (count | sum R << 32, sum G | sum B << 32)
__device__ __forceinline__ void render_disc_cell(const RenderView &V, const RenderDisc &D, int c, unsigned long long w0, unsigned long long w1,
                                                 unsigned long long *__restrict__ img)
{
    const int u = D.u0 + c % D.bw, v = D.v0 + c / D.bw;   // inside the canvas: the box is clipped
    const int dx = 16 * u + 8 - D.cx, dy = 16 * v + 8 - D.cy;
    if (dx * dx + dy * dy <= D.R * D.R || (u == D.pu && v == D.pv)) {
        const size_t p = ((size_t)v * V.W + u) * 2;
        atomicAdd(&img[p], w0);
        atomicAdd(&img[p + 1], w1);
    }
}

__global__ __launch_bounds__(RND_THREADS) void render_node_small_kernel(RenderView V, RenderNodes N, unsigned long long *__restrict__ img,
                                                                        uint32_t *__restrict__ list, unsigned int *n_list)
{
    const int lane = threadIdx.x % RND_NODE_G;
    const int64_t k = (int64_t)blockIdx.x * (RND_THREADS / RND_NODE_G) + threadIdx.x / RND_NODE_G;
    if (k >= N.n) return;
    RenderDisc D;
    if (!render_disc(V, N, k, D)) return;
    if (D.R > RND_NODE_SMALL_R) {
        if (lane == 0) list[atomicAdd(n_list, 1u)] = (uint32_t)k;
        return;
    }
    const uint8_t *rgb = N.rgb + 3 * k;
    const unsigned long long w0 = 1ull | (unsigned long long)rgb[0] << 32, w1 = (unsigned long long)rgb[1] | (unsigned long long)rgb[2] << 32;
    for (int c = lane; c < D.bw * D.bh; c += RND_NODE_G) render_disc_cell(V, D, c, w0, w1, img);
}

__global__ __launch_bounds__(RND_THREADS) void render_node_large_kernel(RenderView V, RenderNodes N, unsigned long long *__restrict__ img,
                                                                        const uint32_t *__restrict__ list, const unsigned int *n_list)
{
    const unsigned int n = *n_list;
    for (unsigned int j = blockIdx.x; j < n; j += gridDim.x) {
        const int64_t k = list[j];
        RenderDisc D;
        if (!render_disc(V, N, k, D)) continue;
        const uint8_t *rgb = N.rgb + 3 * k;
        const unsigned long long w0 = 1ull | (unsigned long long)rgb[0] << 32, w1 = (unsigned long long)rgb[1] | (unsigned long long)rgb[2] << 32;
        for (int c = threadIdx.x; c < D.bw * D.bh; c += RND_THREADS) render_disc_cell(V, D, c, w0, w1, img);
    }
}

__global__ __launch_bounds__(RND_THREADS) void render_compose_kernel(const unsigned int *__restrict__ edge, const unsigned long long *__restrict__ node,
                                                                     int64_t n_px, uchar4 ce_rgb, const uint8_t *__restrict__ lut_e, unsigned int Le,
                                                                     const uint8_t *__restrict__ lut_n, unsigned int Ln, uchar4 *__restrict__ out)
{
    const int64_t p = (int64_t)blockIdx.x * RND_THREADS + threadIdx.x;
    if (p >= n_px) return;
    const unsigned int ce = edge[p];
    const unsigned long long n0 = node[2 * p], n1 = node[2 * p + 1];
    const unsigned int cn = (unsigned int)n0;
    const unsigned int Ae = lut_e[min(ce, Le - 1)], An = lut_n[min(cn, Ln - 1)];
    unsigned int Cn[3] = {0, 0, 0};
    if (cn) {
        const unsigned long long sum[3] = {n0 >> 32, n1 & 0xFFFFFFFFull, n1 >> 32};
        for (int k = 0; k < 3; ++k) Cn[k] = (unsigned int)((sum[k] + cn / 2) / cn);
    }
    const unsigned int t = Ae * (255 - An), den = 255 * An + t;
    const unsigned int Ce[3] = {ce_rgb.x, ce_rgb.y, ce_rgb.z};
    unsigned int C[3] = {0, 0, 0};
    if (den)
        for (int k = 0; k < 3; ++k) C[k] = (255 * An * Cn[k] + t * Ce[k] + den / 2) / den;
    out[p] = make_uchar4((unsigned char)C[0], (unsigned char)C[1], (unsigned char)C[2], (unsigned char)((den + 127) / 255));
}

static unsigned render_grid(int64_t n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

}  // namespace nabo

using nabo::DevBuf;

namespace {
enum { RND_MS_CLEAR, RND_MS_EDGES, RND_MS_NODES, RND_MS_COMPOSE, RND_MS_TOTAL };
}

struct nabo_canvas {
    int device = 0;
    nabo::RenderView V = {};
    int64_t chunk = nabo::RND_CHUNK;
    uint64_t n_points = 0;
    int64_t n_nodes = 0;
    DevBuf edge, node, pts, last, list, n_list, xy, rad, rgb, lut_e, lut_n, out;
    hipEvent_t ev[2] = {};
    double ms[5] = {0, 0, 0, 0, 0};
    ~nabo_canvas()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    size_t px() const { return (size_t)V.W * V.H; }
};

namespace {

int render_enter(nabo_canvas *C)
{
    if (!C) return nabo::api_fail(NABO_E_INVALID, "canvas is NULL");
    return nabo::use_device(C->device);
}

int render_clear(nabo_canvas *C)
{
    for (double &m : C->ms) m = 0;
    C->n_points = 0;
    C->n_nodes = 0;
    nabo::PhaseTimer T{C->ev, C->ms, RND_MS_TOTAL};
    int rc = T.start();
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(C->edge.p, 0, C->px() * 4, nullptr));
    HIP_TRY(hipMemsetAsync(C->node.p, 0, C->px() * 16, nullptr));
    return T.stop(RND_MS_CLEAR);
}

// the points P (on the device) through the two edge kernels
int render_draw_points(nabo_canvas *C, const nabo::RenderPts &P)
{
    if (P.n == 0) return NABO_OK;
    int rc = C->list.reserve((size_t)P.n * 4);
    if (rc) return rc;
    nabo::PhaseTimer T{C->ev, C->ms, RND_MS_TOTAL};
    if ((rc = T.start())) return rc;
    HIP_TRY(hipMemsetAsync(C->n_list.p, 0, 4, nullptr));
    hipLaunchKernelGGL(nabo::render_edge_short_kernel, dim3(nabo::render_grid(P.n, nabo::RND_THREADS / nabo::RND_EDGE_G)), dim3(nabo::RND_THREADS), 0,
                       nullptr, C->V, P, C->edge.as<unsigned int>(), C->list.as<uint32_t>(), C->n_list.as<unsigned int>());
    HIP_TRY(hipGetLastError());
    const unsigned lg = std::min<unsigned>(nabo::RND_LONG_GRID, nabo::render_grid(P.n, nabo::RND_THREADS / 64));
    hipLaunchKernelGGL(nabo::render_edge_long_kernel, dim3(lg), dim3(nabo::RND_THREADS), 0, nullptr, C->V, P, C->edge.as<unsigned int>(),
                       C->list.as<uint32_t>(), C->n_list.as<unsigned int>());
    HIP_TRY(hipGetLastError());
    return T.stop(RND_MS_EDGES);
}

int render_count_points(nabo_canvas *C, uint64_t np)
{
    if (np > nabo::RND_MAX_POINTS - C->n_points)
        return nabo::api_fail(NABO_E_INVALID, "%llu points after %llu since the last clear: a pixel's count could pass 2^32 - 1",
                              (unsigned long long)np, (unsigned long long)C->n_points);
    return NABO_OK;
}

// host points [np][2] and their last-marks, at most max_chunk of them at a time
int render_upload_points(nabo_canvas *C, int64_t np, const double *points, const uint8_t *last, int64_t max_chunk)
{
    const int64_t chunk = std::min(max_chunk, np);
    int rc = C->pts.reserve((size_t)(chunk + 1) * 16);
    if (rc || (rc = C->last.reserve((size_t)chunk))) return rc;
    nabo::RenderPts P = {};
    P.pts = C->pts.as<double2>();
    P.last = C->last.as<uint8_t>();
    for (int64_t g0 = 0; g0 < np; g0 += chunk) {
        const int64_t g1 = std::min(np, g0 + chunk), upto = std::min(np, g1 + 1);
        HIP_TRY(hipMemcpy(C->pts.p, points + 2 * g0, (size_t)(upto - g0) * 16, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(C->last.p, last + g0, (size_t)(g1 - g0), hipMemcpyHostToDevice));
        P.n = g1 - g0;
        if ((rc = render_draw_points(C, P))) return rc;
    }
    return NABO_OK;
}

int render_add_nodes(nabo_canvas *C, int64_t n, const double *x, const double *y, const uint16_t *radius, const uint8_t *rgb)
{
    const int64_t chunk = std::min(C->chunk, n);
    int rc = C->xy.reserve((size_t)chunk * 16);
    if (rc || (rc = C->rad.reserve((size_t)chunk * 2)) || (rc = C->rgb.reserve((size_t)chunk * 3)) || (rc = C->list.reserve((size_t)chunk * 4))) return rc;
    std::vector<double> xy((size_t)chunk * 2);
    nabo::RenderNodes N = {C->xy.as<double2>(), C->rad.as<uint16_t>(), C->rgb.as<uint8_t>(), 0};
    nabo::PhaseTimer T{C->ev, C->ms, RND_MS_TOTAL};
    for (int64_t k0 = 0; k0 < n; k0 += chunk) {
        const int64_t nc = std::min(chunk, n - k0);
        for (int64_t k = 0; k < nc; ++k) {
            xy[(size_t)2 * k] = x[k0 + k];
            xy[(size_t)2 * k + 1] = y[k0 + k];
        }
        HIP_TRY(hipMemcpy(C->xy.p, xy.data(), (size_t)nc * 16, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(C->rad.p, radius + k0, (size_t)nc * 2, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(C->rgb.p, rgb + 3 * k0, (size_t)nc * 3, hipMemcpyHostToDevice));
        N.n = nc;
        if ((rc = T.start())) return rc;
        HIP_TRY(hipMemsetAsync(C->n_list.p, 0, 4, nullptr));
        hipLaunchKernelGGL(nabo::render_node_small_kernel, dim3(nabo::render_grid(nc, nabo::RND_THREADS / nabo::RND_NODE_G)), dim3(nabo::RND_THREADS), 0,
                           nullptr, C->V, N, C->node.as<unsigned long long>(), C->list.as<uint32_t>(), C->n_list.as<unsigned int>());
        HIP_TRY(hipGetLastError());
        const unsigned lg = (unsigned)std::min<int64_t>(nabo::RND_LONG_GRID, nc);
        hipLaunchKernelGGL(nabo::render_node_large_kernel, dim3(lg), dim3(nabo::RND_THREADS), 0, nullptr, C->V, N, C->node.as<unsigned long long>(),
                           C->list.as<uint32_t>(), C->n_list.as<unsigned int>());
        HIP_TRY(hipGetLastError());
        if ((rc = T.stop(RND_MS_NODES))) return rc;
    }
    return NABO_OK;
}

int render_create(nabo_canvas *C, int W, int H, double x0, double x1, double y0, double y1)
{
    C->V = {W, H, x0, x1 - x0, y0, y1 - y0};
    HIP_TRY(C->edge.alloc(C->px() * 4));
    HIP_TRY(C->node.alloc(C->px() * 16));
    HIP_TRY(C->n_list.alloc(8));
    for (hipEvent_t &e : C->ev) HIP_TRY(hipEventCreate(&e));
    return render_clear(C);
}

void render_lut(double alpha, int L, uint8_t *lut)
{
    const double k = 1.0 - alpha;
    double t = 1.0;
    for (int c = 0; c < L; ++c) {
        lut[c] = (uint8_t)std::floor(255.0 * (1.0 - t) + 0.5);
        t = t * k;
    }
}

// the node image, [px][2] words, on the host
int render_node_words(nabo_canvas *C, std::vector<unsigned long long> &w)
{
    w.resize(C->px() * 2);
    HIP_TRY(hipMemcpy(w.data(), C->node.p, w.size() * 8, hipMemcpyDeviceToHost));
    return NABO_OK;
}

}  // namespace

extern "C" {

int nabo_render_geometry(int32_t *subpixel_bits, int32_t *r_max, int32_t *edge_short_steps, int32_t *edge_group, int32_t *node_small_r,
                         int32_t *node_group)
{
    if (subpixel_bits) *subpixel_bits = nabo::RND_SUB_BITS;
    if (r_max) *r_max = nabo::RND_R_MAX;
    if (edge_short_steps) *edge_short_steps = nabo::RND_EDGE_SHORT;
    if (edge_group) *edge_group = nabo::RND_EDGE_G;
    if (node_small_r) *node_small_r = nabo::RND_NODE_SMALL_R;
    if (node_group) *node_group = nabo::RND_NODE_G;
    return NABO_OK;
}

int nabo_render_alpha_lut(double alpha, int32_t L, uint8_t *lut)
{
    if (!lut) return nabo::api_fail(NABO_E_INVALID, "lut is NULL");
    if (!(alpha >= 0.0 && alpha <= 1.0)) return nabo::api_fail(NABO_E_INVALID, "alpha=%g must be in [0, 1]", alpha);
    if (L < 2 || L > nabo::RND_MAX_LUT) return nabo::api_fail(NABO_E_INVALID, "L=%d must be in [2, %d]", L, nabo::RND_MAX_LUT);
    render_lut(alpha, L, lut);
    return NABO_OK;
}

int nabo_render_create(nabo_canvas **out, int32_t device, int32_t W, int32_t H, double x0, double x1, double y0, double y1)
{
    if (!out) return nabo::api_fail(NABO_E_INVALID, "out is NULL");
    *out = nullptr;
    if (W < 1 || W > nabo::RND_MAX_SIDE || H < 1 || H > nabo::RND_MAX_SIDE)
        return nabo::api_fail(NABO_E_INVALID, "W=%d and H=%d must be in [1, %d]", W, H, nabo::RND_MAX_SIDE);
    if (!std::isfinite(x0) || !std::isfinite(x1) || !std::isfinite(y0) || !std::isfinite(y1) || !(x0 < x1) || !(y0 < y1) ||
        !std::isfinite(x1 - x0) || !std::isfinite(y1 - y0))
        return nabo::api_fail(NABO_E_INVALID, "the viewport (%g, %g, %g, %g) must be finite with x0 < x1 and y0 < y1", x0, x1, y0, y1);
    int rc = nabo::use_device(device);
    if (rc) return rc;
    return nabo::create_handle(out, device, "nabo_render_create", [&](nabo_canvas *C) { return render_create(C, W, H, x0, x1, y0, y1); });
}

void nabo_render_destroy(nabo_canvas *C)
{
    if (!C) return;
    (void)hipSetDevice(C->device);
    delete C;
}

int nabo_render_clear(nabo_canvas *C)
{
    int rc = render_enter(C);
    return rc ? rc : render_clear(C);
}

int nabo_render_set_option(nabo_canvas *C, const char *name, int64_t value)
{
    if (!C || !name) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    if (strcmp(name, "chunk_points") != 0) return nabo::api_fail(NABO_E_INVALID, "unknown canvas option %s", name);
    if (value < 1 || value > nabo::RND_MAX_CHUNK) return nabo::api_fail(NABO_E_INVALID, "chunk_points=%lld must be in [1, 2^28]", (long long)value);
    C->chunk = value;
    return NABO_OK;
}

int nabo_render_add_polylines(nabo_canvas *C, int64_t n_lines, const int64_t *offsets, const double *points)
{
    int rc = render_enter(C);
    if (rc) return rc;
    if (n_lines < 0) return nabo::api_fail(NABO_E_INVALID, "n_lines=%lld is negative", (long long)n_lines);
    if (n_lines == 0) return NABO_OK;
    if (!offsets || !points) return nabo::api_fail(NABO_E_INVALID, "offsets or points is NULL");
    if (offsets[0] != 0) return nabo::api_fail(NABO_E_INVALID, "offsets[0] = %lld, must be 0", (long long)offsets[0]);
    for (int64_t e = 0; e < n_lines; ++e)
        if (offsets[e + 1] - offsets[e] < 2 || offsets[e + 1] < offsets[e])
            return nabo::api_fail(NABO_E_INVALID, "polyline %lld has %lld points, must be at least 2", (long long)e, (long long)(offsets[e + 1] - offsets[e]));
    const int64_t np = offsets[n_lines];
    for (int64_t i = 0; i < 2 * np; ++i)
        if (!std::isfinite(points[i])) return nabo::api_fail(NABO_E_INVALID, "coordinate %lld is not finite", (long long)i);
    if ((rc = render_count_points(C, (uint64_t)np))) return rc;
    try {
        std::vector<uint8_t> last((size_t)np, 0);
        for (int64_t e = 0; e < n_lines; ++e) last[(size_t)offsets[e + 1] - 1] = 1;
        if ((rc = render_upload_points(C, np, points, last.data(), C->chunk))) return rc;
    } catch (const std::bad_alloc &) {
        return nabo::api_fail(NABO_E_NOMEM, "nabo_render_add_polylines: out of host memory");
    }
    C->n_points += (uint64_t)np;
    return NABO_OK;
}

int nabo_render_add_edges(nabo_canvas *C, int64_t n, const double *x, const double *y, int64_t n_edges, const int64_t *src, const int64_t *dst)
{
    int rc = render_enter(C);
    if (rc) return rc;
    if (n < 0 || n_edges < 0) return nabo::api_fail(NABO_E_INVALID, "n=%lld or n_edges=%lld is negative", (long long)n, (long long)n_edges);
    if (n_edges == 0) return NABO_OK;
    if (!x || !y || !src || !dst) return nabo::api_fail(NABO_E_INVALID, "x, y, src or dst is NULL");
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(x[i]) || !std::isfinite(y[i])) return nabo::api_fail(NABO_E_INVALID, "the position of node %lld is not finite", (long long)i);
    for (int64_t e = 0; e < n_edges; ++e)
        if (src[e] < 0 || src[e] >= n || dst[e] < 0 || dst[e] >= n)
            return nabo::api_fail(NABO_E_INVALID, "edge %lld = (%lld, %lld) names a node outside [0, %lld)", (long long)e, (long long)src[e],
                                  (long long)dst[e], (long long)n);
    if ((uint64_t)n_edges > nabo::RND_MAX_POINTS / 2) return nabo::api_fail(NABO_E_INVALID, "%lld edges are more than 2^31 - 1", (long long)n_edges);
    if ((rc = render_count_points(C, 2 * (uint64_t)n_edges))) return rc;
    try {
        // whole edges per upload: a chunk of 1 point still takes one edge
        const int64_t ce = std::min(n_edges, std::max<int64_t>(1, C->chunk / 2));
        std::vector<double> pts((size_t)ce * 4);
        std::vector<uint8_t> last((size_t)ce * 2);
        for (int64_t e = 0; e < ce; ++e) last[(size_t)2 * e] = 0, last[(size_t)2 * e + 1] = 1;
        for (int64_t e0 = 0; e0 < n_edges; e0 += ce) {
            const int64_t nc = std::min(ce, n_edges - e0);
            for (int64_t e = 0; e < nc; ++e) {
                pts[(size_t)4 * e] = x[src[e0 + e]];
                pts[(size_t)4 * e + 1] = y[src[e0 + e]];
                pts[(size_t)4 * e + 2] = x[dst[e0 + e]];
                pts[(size_t)4 * e + 3] = y[dst[e0 + e]];
            }
            if ((rc = render_upload_points(C, 2 * nc, pts.data(), last.data(), 2 * ce))) return rc;
        }
    } catch (const std::bad_alloc &) {
        return nabo::api_fail(NABO_E_NOMEM, "nabo_render_add_edges: out of host memory");
    }
    C->n_points += 2 * (uint64_t)n_edges;
    return NABO_OK;
}

int nabo_render_add_bundle(nabo_canvas *C, nabo_bundle *B)
{
    int rc = render_enter(C);
    if (rc) return rc;
    if (!B) return nabo::api_fail(NABO_E_INVALID, "bundle is NULL");
    const nabo::BundleView bv = nabo::bundle_view(B);
    if (bv.device != C->device) return nabo::api_fail(NABO_E_INVALID, "the bundle lives on device %d, the canvas on device %d", bv.device, C->device);
    if ((rc = render_count_points(C, (uint64_t)bv.n_points))) return rc;
    if ((rc = C->last.reserve((size_t)bv.n_points))) return rc;
    HIP_TRY(hipMemsetAsync(C->last.p, 0, (size_t)bv.n_points, nullptr));
    hipLaunchKernelGGL(nabo::render_mark_kernel, dim3(nabo::render_grid(bv.n_edges, nabo::RND_THREADS)), dim3(nabo::RND_THREADS), 0, nullptr, bv.off,
                       bv.n_edges, C->last.as<uint8_t>());
    HIP_TRY(hipGetLastError());
    nabo::RenderPts P = {};
    P.denorm = 1;
    for (int a = 0; a < 2; ++a) P.lo[a] = bv.lo[a], P.span[a] = bv.span[a];
    for (int64_t g0 = 0; g0 < bv.n_points; g0 += C->chunk) {
        P.pts = reinterpret_cast<const double2 *>(bv.pts) + g0;
        P.last = C->last.as<uint8_t>() + g0;
        P.n = std::min(C->chunk, bv.n_points - g0);
        if ((rc = render_draw_points(C, P))) return rc;
    }
    C->n_points += (uint64_t)bv.n_points;
    return NABO_OK;
}

int nabo_render_add_nodes(nabo_canvas *C, int64_t n, const double *x, const double *y, const uint16_t *radius, const uint8_t *rgb)
{
    int rc = render_enter(C);
    if (rc) return rc;
    if (n < 0) return nabo::api_fail(NABO_E_INVALID, "n=%lld is negative", (long long)n);
    if (n == 0) return NABO_OK;
    if (!x || !y || !radius || !rgb) return nabo::api_fail(NABO_E_INVALID, "x, y, radius or rgb is NULL");
    for (int64_t i = 0; i < n; ++i) {
        if (!std::isfinite(x[i]) || !std::isfinite(y[i])) return nabo::api_fail(NABO_E_INVALID, "the position of node %lld is not finite", (long long)i);
        if (radius[i] > nabo::RND_R_MAX)
            return nabo::api_fail(NABO_E_INVALID, "radius[%lld] = %d/16 pixel is more than R_MAX = %d", (long long)i, (int)radius[i], nabo::RND_R_MAX);
    }
    if (n > nabo::RND_MAX_NODES - C->n_nodes)
        return nabo::api_fail(NABO_E_INVALID, "%lld nodes after %lld since the last clear are more than 2^24", (long long)n, (long long)C->n_nodes);
    try {
        if ((rc = render_add_nodes(C, n, x, y, radius, rgb))) return rc;
    } catch (const std::bad_alloc &) {
        return nabo::api_fail(NABO_E_NOMEM, "nabo_render_add_nodes: out of host memory");
    }
    C->n_nodes += n;
    return NABO_OK;
}

int nabo_render_edge_counts(nabo_canvas *C, uint32_t *counts)
{
    int rc = render_enter(C);
    if (rc) return rc;
    if (counts) HIP_TRY(hipMemcpy(counts, C->edge.p, C->px() * 4, hipMemcpyDeviceToHost));
    return NABO_OK;
}

int nabo_render_node_counts(nabo_canvas *C, uint32_t *counts)
{
    int rc = render_enter(C);
    if (rc || !counts) return rc;
    try {
        std::vector<unsigned long long> w;
        if ((rc = render_node_words(C, w))) return rc;
        for (size_t p = 0; p < C->px(); ++p) counts[p] = (uint32_t)w[2 * p];
    } catch (const std::bad_alloc &) {
        return nabo::api_fail(NABO_E_NOMEM, "nabo_render_node_counts: out of host memory");
    }
    return NABO_OK;
}

int nabo_render_node_sums(nabo_canvas *C, uint32_t *sums)
{
    int rc = render_enter(C);
    if (rc || !sums) return rc;
    try {
        std::vector<unsigned long long> w;
        if ((rc = render_node_words(C, w))) return rc;
        for (size_t p = 0; p < C->px(); ++p) {
            sums[3 * p] = (uint32_t)(w[2 * p] >> 32);
            sums[3 * p + 1] = (uint32_t)w[2 * p + 1];
            sums[3 * p + 2] = (uint32_t)(w[2 * p + 1] >> 32);
        }
    } catch (const std::bad_alloc &) {
        return nabo::api_fail(NABO_E_NOMEM, "nabo_render_node_sums: out of host memory");
    }
    return NABO_OK;
}

int nabo_render_compose(nabo_canvas *C, const uint8_t *edge_rgb, const uint8_t *lut_e, int32_t Le, const uint8_t *lut_n, int32_t Ln, uint8_t *out)
{
    int rc = render_enter(C);
    if (rc) return rc;
    if (!edge_rgb || !lut_e || !lut_n || !out) return nabo::api_fail(NABO_E_INVALID, "edge_rgb, lut_e, lut_n or out is NULL");
    if (Le < 2 || Le > nabo::RND_MAX_LUT || Ln < 2 || Ln > nabo::RND_MAX_LUT)
        return nabo::api_fail(NABO_E_INVALID, "Le=%d and Ln=%d must be in [2, %d]", Le, Ln, nabo::RND_MAX_LUT);
    if ((rc = C->lut_e.reserve((size_t)Le)) || (rc = C->lut_n.reserve((size_t)Ln)) || (rc = C->out.reserve(C->px() * 4))) return rc;
    HIP_TRY(hipMemcpy(C->lut_e.p, lut_e, (size_t)Le, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(C->lut_n.p, lut_n, (size_t)Ln, hipMemcpyHostToDevice));
    nabo::PhaseTimer T{C->ev, C->ms, RND_MS_TOTAL};
    if ((rc = T.start())) return rc;
    hipLaunchKernelGGL(nabo::render_compose_kernel, dim3(nabo::render_grid((int64_t)C->px(), nabo::RND_THREADS)), dim3(nabo::RND_THREADS), 0, nullptr,
                       C->edge.as<unsigned int>(), C->node.as<unsigned long long>(), (int64_t)C->px(), make_uchar4(edge_rgb[0], edge_rgb[1], edge_rgb[2], 0),
                       C->lut_e.as<uint8_t>(), (unsigned int)Le, C->lut_n.as<uint8_t>(), (unsigned int)Ln, C->out.as<uchar4>());
    HIP_TRY(hipGetLastError());
    if ((rc = T.stop(RND_MS_COMPOSE))) return rc;
    HIP_TRY(hipMemcpy(out, C->out.p, C->px() * 4, hipMemcpyDeviceToHost));
    return NABO_OK;
}

int nabo_render_last_ms(nabo_canvas *C, double ms[5])
{
    if (!C || !ms) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    for (int i = 0; i < 5; ++i) ms[i] = C->ms[i];
    return NABO_OK;
}

}  // extern "C"
