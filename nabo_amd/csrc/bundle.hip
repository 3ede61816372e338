// Edge bundling by density-guided advection (include/nabo_bundle.h is the contract and holds the definition;
// nabo/_graphplot.py:192-220, datashader's hammer_bundle, is what it replaces).
//
// The state is the packed polylines: offsets [E+1] and points (16 B each), two copies that the steps ping-pong between.
// A round (a resample, or s advection steps with their resamples) runs in ONE launch per class of edge: within a round
// the edges are coupled only through the field, so a group of lanes keeps its edge in LDS from the first step to the last.
//   short kernel: BND_SHORT_G = 8 lanes per edge, 32 edges per workgroup, room for BND_SHORT_CAP = 16 points.  In an SNN
//     graph on a layout most edges are shorter than one target segment and stay at two points for ever: an edge that a
//     resample leaves at two points is done for the round (its end points never move, and resampling them returns them).
//   long kernel: one wave per edge, room for 2 * P_MAX points.  It takes the edges the short kernel gave up: those that
//     start with more than BND_SHORT_CAP points or whose resample asks for more.  The short kernel appends them to a list
//     with an integer atomic; the list's order decides nothing, because every edge has its own result slot and both
//     kernels run the same device function, operation for operation.
// Output offsets: a bounded slot per edge plus compaction.  A chunk of edges (option chunk_edges) gets P_MAX-point slots;
// the kernels write points and a count per edge, a one-workgroup scan turns the counts into offsets that continue the
// previous chunk's, and a copy packs the slots.  The host reads the running total (8 bytes) once per chunk to make
// room.  Offsets are therefore a function of the counts alone.
// Density: device-scope integer atomicAdd, one per point (exact in any order).  The field is four small kernels over the
// image (two blurs, the second of which also takes the maximum by an integer atomicMax of the bits of a non-negative
// double, then gradient and normalisation); GX and GY are stored as one 16-byte pair per pixel.
// Bounds: a pixel index is clamped to [0, A]; set_points takes only coordinates in [0, 1] and 2 .. 2 * P_MAX points per
// edge; a resample writes at most min(capacity, P_MAX) points or gives the edge up before writing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/nabo_bundle.h"
#include "bundle_view.h"
#include "host_common.h"

#pragma clang fp contract(off)

namespace nabo {

constexpr int BND_PMAX = 256;
constexpr int BND_IN_MAX = 2 * BND_PMAX;   // points an edge may hold on entry (set_points)
constexpr int BND_SHORT_G = 8, BND_SHORT_CAP = 16, BND_SHORT_THREADS = 256;
constexpr int BND_SHORT_EDGES = BND_SHORT_THREADS / BND_SHORT_G;
constexpr int BND_LONG_G = 64, BND_LONG_THREADS = 128;
constexpr int BND_LONG_EDGES = BND_LONG_THREADS / BND_LONG_G;
constexpr int BND_LONG_GRID = 2048;
constexpr int BND_THREADS = 256;
constexpr int BND_SCAN_THREADS = 1024;
constexpr int BND_COPY_G = 16;
constexpr int64_t BND_CHUNK = 262144;   // edges per chunk by default: 1 GiB of slots (a graph of fewer edges takes what it needs)

struct BundleRound {
    const int64_t *off;
    const double2 *pts;
    int64_t e0, e1;
    const double2 *field;
    int A, n_steps, resample_every;   // n_steps == 0: one resample and no step
    double tl;
    double2 *slot;       // [e1 - e0][BND_PMAX]
    int32_t *cnt;        // [e1 - e0]
    int32_t *redo;       // [e1 - e0]: the edges (relative to e0) left to the long kernel
    unsigned int *n_redo;
};

// the lanes of a group are lanes of one wave: LDS operations of a wave complete in order, so what is needed is that the
// compiler keeps them in order and waits for them
__device__ __forceinline__ void bundle_group_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// Resample P[0 .. p) into Q; the number of points written, or -1 (nothing written) if that exceeds OUT_CAP.
template <int G, int OUT_CAP>
__device__ __forceinline__ int bundle_resample(const double2 *P, int p, double2 *Q, double *__restrict__ c, double *__restrict__ sg, double tl,
                                               int lane)
{
    for (int j = lane; j < p - 1; j += G) {
        const double dx = P[j + 1].x - P[j].x, dy = P[j + 1].y - P[j].y;
        sg[j] = __dsqrt_rn(dx * dx + dy * dy);
    }
    bundle_group_sync();
    if (lane == 0) {
        double a = 0.0;
        c[0] = 0.0;
#pragma unroll 8
        for (int j = 0; j < p - 1; ++j) {   // (the reads of sg do not wait for the chain of additions)
            a = a + sg[j];
            c[j + 1] = a;
        }
    }
    bundle_group_sync();
    const double L = c[p - 1];
    int m = 2;
    if (L > 0.0) {
        const double r = ceil(L / tl) + 1.0;
        m = r >= (double)BND_PMAX ? BND_PMAX : (int)r;
    }
    if (m > OUT_CAP) return -1;
    const double step = L / (double)(m - 1);
    for (int i = lane; i < m; i += G) {
        double2 q;
        if (i == 0)
            q = P[0];
        else if (i == m - 1)
            q = P[p - 1];
        else {
            const double t = (double)i * step;
            int lo = 0, hi = p - 1;   // c[lo] <= t; the answer is in [lo, hi)
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (c[mid] <= t) lo = mid;
                else hi = mid;
            }
            const double s = sg[lo];
            const double f = s == 0.0 ? 0.0 : (t - c[lo]) / s;
            const double2 a = P[lo], b = P[lo + 1];
            q.x = a.x + (b.x - a.x) * f;
            q.y = a.y + (b.y - a.y) * f;
        }
        Q[i] = q;
    }
    bundle_group_sync();
    return m;
}

__device__ __forceinline__ int bundle_pixel(double q, double Ad, int A)
{
    const int u = (int)(q * Ad);
    return min(max(u, 0), A);
}

// One edge through a round, in LDS; the points it ends with are written to its slot.  Returns their number, or -1 if the
// edge does not fit CAP points (nothing is written then).
template <int G, int CAP>
__device__ __forceinline__ int bundle_edge(const BundleRound &R, int64_t e, double2 *cur, double2 *nxt, double *c, double *sg, int lane)
{
    constexpr int OUT_CAP = CAP < BND_PMAX ? CAP : BND_PMAX;
    const int64_t o = R.off[e];
    int p = (int)(R.off[e + 1] - o);
    if (p > CAP) return -1;
    for (int j = lane; j < p; j += G) cur[j] = R.pts[o + j];
    bundle_group_sync();
    if (R.n_steps == 0) {
        const int m = bundle_resample<G, OUT_CAP>(cur, p, nxt, c, sg, R.tl, lane);
        if (m < 0) return -1;
        double2 *t = cur;
        cur = nxt;
        nxt = t;
        p = m;
    }
    const double Ad = (double)R.A;
    const size_t A1 = (size_t)R.A + 1;
    for (int s = 1; s <= R.n_steps; ++s) {
        // a lane moves the same points in every step between two resamples: no exchange until the resample
        for (int j = lane; j < p - 1; j += G) {
            if (j == 0) continue;
            double2 q = cur[j];
            const int u = bundle_pixel(q.x, Ad, R.A), v = bundle_pixel(q.y, Ad, R.A);
            const double2 g = R.field[(size_t)u * A1 + (size_t)v];
            q.x = fmin(fmax(q.x + g.x / Ad, 0.0), 1.0);
            q.y = fmin(fmax(q.y + g.y / Ad, 0.0), 1.0);
            cur[j] = q;
        }
        if (s % R.resample_every == 0 || s == R.n_steps) {
            bundle_group_sync();
            const int m = bundle_resample<G, OUT_CAP>(cur, p, nxt, c, sg, R.tl, lane);
            if (m < 0) return -1;
            double2 *t = cur;
            cur = nxt;
            nxt = t;
            p = m;
            if (p == 2) break;   // two end points: no step moves them, and every later resample returns them as they are
        }
    }
    double2 *out = R.slot + (size_t)(e - R.e0) * BND_PMAX;
    for (int j = lane; j < p; j += G) out[j] = cur[j];
    return p;
}

__global__ __launch_bounds__(BND_SHORT_THREADS) void bundle_short_kernel(BundleRound R)
{
    __shared__ double2 bufA[BND_SHORT_EDGES][BND_SHORT_CAP], bufB[BND_SHORT_EDGES][BND_SHORT_CAP];
    __shared__ double c[BND_SHORT_EDGES][BND_SHORT_CAP], sg[BND_SHORT_EDGES][BND_SHORT_CAP];
    const int g = threadIdx.x / BND_SHORT_G, lane = threadIdx.x % BND_SHORT_G;
    const int64_t e = R.e0 + (int64_t)blockIdx.x * BND_SHORT_EDGES + g;
    if (e >= R.e1) return;
    const int m = bundle_edge<BND_SHORT_G, BND_SHORT_CAP>(R, e, bufA[g], bufB[g], c[g], sg[g], lane);
    if (lane != 0) return;
    if (m < 0) R.redo[atomicAdd(R.n_redo, 1u)] = (int32_t)(e - R.e0);
    else R.cnt[e - R.e0] = m;
}

__global__ __launch_bounds__(BND_LONG_THREADS) void bundle_long_kernel(BundleRound R)
{
    __shared__ double2 bufA[BND_LONG_EDGES][BND_IN_MAX], bufB[BND_LONG_EDGES][BND_IN_MAX];
    __shared__ double c[BND_LONG_EDGES][BND_IN_MAX], sg[BND_LONG_EDGES][BND_IN_MAX];
    const int g = threadIdx.x / BND_LONG_G, lane = threadIdx.x % BND_LONG_G;
    const unsigned int n = *R.n_redo;
    for (unsigned int k = blockIdx.x * BND_LONG_EDGES + g; k < n; k += gridDim.x * BND_LONG_EDGES) {
        const int64_t e = R.e0 + R.redo[k];
        const int m = bundle_edge<BND_LONG_G, BND_IN_MAX>(R, e, bufA[g], bufB[g], c[g], sg[g], lane);
        if (lane == 0) R.cnt[e - R.e0] = m;   // never -1: set_points admits no more than BND_IN_MAX points
        bundle_group_sync();
    }
}

// offsets of a chunk from its counts, continuing at *total; one workgroup
__global__ __launch_bounds__(BND_SCAN_THREADS) void bundle_scan_kernel(const int32_t *__restrict__ cnt, int64_t nc, int64_t e0,
                                                                       int64_t *__restrict__ off_out, int64_t *__restrict__ total)
{
    __shared__ int64_t part[BND_SCAN_THREADS];
    const int t = threadIdx.x;
    const int64_t base = *total;
    const int64_t per = (nc + BND_SCAN_THREADS - 1) / BND_SCAN_THREADS;
    const int64_t i0 = std::min<int64_t>(nc, t * per), i1 = std::min<int64_t>(nc, i0 + per);
    int64_t s = 0;
    for (int64_t i = i0; i < i1; ++i) s += cnt[i];
    part[t] = s;
    __syncthreads();
    for (int h = 1; h < BND_SCAN_THREADS; h <<= 1) {
        const int64_t add = t >= h ? part[t - h] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    int64_t run = base + part[t] - s;
    for (int64_t i = i0; i < i1; ++i) {
        off_out[e0 + i] = run;
        run += cnt[i];
    }
    if (t == BND_SCAN_THREADS - 1) {
        off_out[e0 + nc] = base + part[t];
        *total = base + part[t];
    }
}

__global__ __launch_bounds__(BND_THREADS) void bundle_copy_kernel(const double2 *__restrict__ slot, const int32_t *__restrict__ cnt,
                                                                  int64_t nc, int64_t e0, const int64_t *__restrict__ off_out,
                                                                  double2 *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * (BND_THREADS / BND_COPY_G) + threadIdx.x / BND_COPY_G;
    if (i >= nc) return;
    const int m = cnt[i];
    const double2 *s = slot + (size_t)i * BND_PMAX;
    double2 *d = out + off_out[e0 + i];
    for (int j = threadIdx.x % BND_COPY_G; j < m; j += BND_COPY_G) d[j] = s[j];
}

__global__ __launch_bounds__(BND_THREADS) void bundle_density_kernel(const double2 *__restrict__ pts, int64_t n, int A,
                                                                     unsigned int *__restrict__ img)
{
    const double Ad = (double)A;
    const size_t A1 = (size_t)A + 1;
    for (int64_t i = (int64_t)blockIdx.x * BND_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * BND_THREADS) {
        const double2 q = pts[i];
        atomicAdd(&img[(size_t)bundle_pixel(q.x, Ad, A) * A1 + (size_t)bundle_pixel(q.y, Ad, A)], 1u);
    }
}

// one axis of the blur; with mx, also the maximum of the outputs (the bits of a non-negative double order as integers)
template <typename T>
__global__ __launch_bounds__(BND_THREADS) void bundle_blur_kernel(const T *__restrict__ in, double *__restrict__ out, int A, int R,
                                                                  const double *__restrict__ w, int axis, unsigned long long *mx)
{
    const int A1 = A + 1;
    const int64_t idx = (int64_t)blockIdx.x * BND_THREADS + threadIdx.x;
    double acc = 0.0;
    if (idx < (int64_t)A1 * A1) {
        const int u = (int)(idx / A1), v = (int)(idx % A1);
        const int pos = axis == 0 ? u : v;
        const int64_t stride = axis == 0 ? A1 : 1;
        const int t0 = std::max(-R, -pos), t1 = std::min(R, A - pos);
        for (int t = t0; t <= t1; ++t) acc = acc + w[t + R] * (double)in[idx + t * stride];
        out[idx] = acc;
    }
    if (mx) {
        for (int o = 32; o > 0; o >>= 1) acc = fmax(acc, __shfl_xor(acc, o, 64));
        if ((threadIdx.x & 63) == 0 && acc > 0.0) atomicMax(mx, (unsigned long long)__double_as_longlong(acc));
    }
}

__global__ __launch_bounds__(BND_THREADS) void bundle_field_kernel(const double *__restrict__ Bl, int A, const unsigned long long *mx,
                                                                   double2 *__restrict__ F)
{
    const int A1 = A + 1;
    const int64_t idx = (int64_t)blockIdx.x * BND_THREADS + threadIdx.x;
    if (idx >= (int64_t)A1 * A1) return;
    const int u = (int)(idx / A1), v = (int)(idx % A1);
    const double m = __longlong_as_double((long long)*mx);
    const int up = std::min(u + 1, A), um = std::max(u - 1, 0), vp = std::min(v + 1, A), vm = std::max(v - 1, 0);
    const double gx = Bl[(int64_t)up * A1 + v] / m - Bl[(int64_t)um * A1 + v] / m;
    const double gy = Bl[(int64_t)u * A1 + vp] / m - Bl[(int64_t)u * A1 + vm] / m;
    const double mag = __dsqrt_rn(gx * gx + gy * gy) + 1e-5;
    F[idx] = make_double2(gx / mag, gy / mag);
}

__global__ __launch_bounds__(BND_THREADS) void bundle_ends_kernel(const int64_t *__restrict__ off, int64_t E, uint8_t *__restrict__ ends)
{
    const int64_t e = (int64_t)blockIdx.x * BND_THREADS + threadIdx.x;
    if (e >= E) return;
    ends[off[e]] = 1;
    ends[off[e + 1] - 1] = 1;
}

__global__ __launch_bounds__(BND_THREADS) void bundle_smooth_kernel(const double2 *__restrict__ in, double2 *__restrict__ out,
                                                                    const uint8_t *__restrict__ ends, int64_t n, double keep, double half)
{
    const int64_t i = (int64_t)blockIdx.x * BND_THREADS + threadIdx.x;
    if (i >= n) return;
    double2 q = in[i];
    if (!ends[i]) {   // an interior point: i - 1 and i + 1 are points of the same edge
        const double2 a = in[i - 1], b = in[i + 1];
        q.x = (keep * q.x) + (half * (a.x + b.x));
        q.y = (keep * q.y) + (half * (a.y + b.y));
    }
    out[i] = q;
}

static unsigned bundle_grid(int64_t n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

}  // namespace nabo

using nabo::DevBuf;

namespace {
enum { BND_MS_RESAMPLE, BND_MS_DENSITY, BND_MS_FIELD, BND_MS_ADVECT, BND_MS_SMOOTH, BND_MS_TOTAL };

struct BundleScalars {   // on the device
    unsigned int n_redo, pad_;
    int64_t total;
    unsigned long long mx;
};

// the weights of nabo_bundle_blur_weights
int bundle_radius(double b) { return (int)std::ceil(4.0 * (b / 2.0)); }
void bundle_weights(double b, int R, double *w)
{
    const double sigma = b / 2.0;
    double sum = 0.0;
    for (int t = -R; t <= R; ++t) {
        const double z = (double)t / sigma;
        w[t + R] = std::exp(-0.5 * (z * z));
        sum = sum + w[t + R];
    }
    for (int t = 0; t <= 2 * R; ++t) w[t] = w[t] / sum;
}
}  // namespace

struct nabo_bundle {
    int device = 0;
    int64_t n = 0, E = 0;
    double lo[2] = {0, 0}, span[2] = {0, 0};
    double initial_bandwidth = 0.05, decay = 0.7, min_seg = 0.008, max_seg = 0.016, tension = 0.3;
    int iterations = 4, A = 500, advect_iterations = 50, resample_every = 2, smooth_passes = 10;
    int64_t chunk = nabo::BND_CHUNK;
    int64_t npts = 0, cap[2] = {0, 0};   // points held, and the room of the two point buffers
    int cur = 0;
    bool have_density = false, have_field = false;
    DevBuf off[2], pts[2], slot, cnt, redo, sc, img, tmp, blur, field, w, ends;
    hipEvent_t ev[2] = {};
    double ms[6] = {0, 0, 0, 0, 0, 0};
    ~nabo_bundle()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

namespace {

// room for `want` points in buffer `which`, keeping its first `keep` points
int bundle_room(nabo_bundle *B, int which, int64_t want, int64_t keep)
{
    if (want <= B->cap[which]) return NABO_OK;
    const int64_t room = want + want / 2 + 1024;
    DevBuf nb;
    if (hipMalloc(&nb.p, (size_t)room * 16) != hipSuccess) {
        nb.p = nullptr;
        (void)hipGetLastError();
        return nabo::api_fail(NABO_E_NOMEM, "no device memory for %lld points", (long long)room);
    }
    nb.cap = (size_t)room * 16;
    if (keep) HIP_TRY(hipMemcpy(nb.p, B->pts[which].p, (size_t)keep * 16, hipMemcpyDeviceToDevice));
    std::swap(B->pts[which].p, nb.p);
    std::swap(B->pts[which].cap, nb.cap);
    B->cap[which] = room;
    return NABO_OK;
}

BundleScalars *bundle_sc(nabo_bundle *B) { return B->sc.as<BundleScalars>(); }

// a resample (n_steps == 0) or a round of n_steps steps, chunk by chunk, from buffer cur into the other one
int bundle_round(nabo_bundle *B, int n_steps)
{
    const int in = B->cur, out = 1 - in;
    const int64_t chunk = std::min(B->chunk, B->E);
    int rc = B->slot.reserve((size_t)chunk * nabo::BND_PMAX * 16);
    if (rc || (rc = B->cnt.reserve((size_t)chunk * 4)) || (rc = B->redo.reserve((size_t)chunk * 4))) return rc;
    if ((rc = bundle_room(B, out, B->npts, 0))) return rc;
    hipStream_t st = nullptr;
    HIP_TRY(hipMemsetAsync(&bundle_sc(B)->total, 0, 8, st));
    nabo::BundleRound R;
    R.off = B->off[in].as<int64_t>();
    R.pts = B->pts[in].as<double2>();
    R.field = B->field.as<double2>();
    R.A = B->A;
    R.n_steps = n_steps;
    R.resample_every = B->resample_every;
    R.tl = (B->min_seg + B->max_seg) / 2.0;
    R.slot = B->slot.as<double2>();
    R.cnt = B->cnt.as<int32_t>();
    R.redo = B->redo.as<int32_t>();
    R.n_redo = &bundle_sc(B)->n_redo;
    int64_t total = 0;
    for (int64_t e0 = 0; e0 < B->E; e0 += chunk) {
        const int64_t nc = std::min(chunk, B->E - e0);
        R.e0 = e0;
        R.e1 = e0 + nc;
        HIP_TRY(hipMemsetAsync(R.n_redo, 0, 4, st));
        hipLaunchKernelGGL(nabo::bundle_short_kernel, dim3(nabo::bundle_grid(nc, nabo::BND_SHORT_EDGES)), dim3(nabo::BND_SHORT_THREADS), 0, st, R);
        HIP_TRY(hipGetLastError());
        const unsigned lg = std::min<unsigned>(nabo::BND_LONG_GRID, nabo::bundle_grid(nc, nabo::BND_LONG_EDGES));
        hipLaunchKernelGGL(nabo::bundle_long_kernel, dim3(lg), dim3(nabo::BND_LONG_THREADS), 0, st, R);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(nabo::bundle_scan_kernel, dim3(1), dim3(nabo::BND_SCAN_THREADS), 0, st, R.cnt, nc, e0,
                           B->off[out].as<int64_t>(), &bundle_sc(B)->total);
        HIP_TRY(hipGetLastError());
        const int64_t before = total;
        HIP_TRY(hipMemcpy(&total, &bundle_sc(B)->total, 8, hipMemcpyDeviceToHost));
        // (the points of this chunk alone are bounded by the slots; the estimate for the rest keeps regrowth rare)
        if (total > B->cap[out] && (rc = bundle_room(B, out, total + 2 * (B->E - R.e1), before))) return rc;
        hipLaunchKernelGGL(nabo::bundle_copy_kernel, dim3(nabo::bundle_grid(nc, nabo::BND_THREADS / nabo::BND_COPY_G)), dim3(nabo::BND_THREADS),
                           0, st, R.slot, R.cnt, nc, e0, B->off[out].as<int64_t>(), B->pts[out].as<double2>());
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(st));
    B->npts = total;
    B->cur = out;
    B->have_density = false;
    return NABO_OK;
}

int bundle_density(nabo_bundle *B)
{
    const size_t px = (size_t)(B->A + 1) * (B->A + 1);
    int rc = B->img.reserve(px * 4);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(B->img.p, 0, px * 4, nullptr));
    const unsigned grid = std::min<unsigned>(2048, nabo::bundle_grid(B->npts, nabo::BND_THREADS));
    hipLaunchKernelGGL(nabo::bundle_density_kernel, dim3(grid), dim3(nabo::BND_THREADS), 0, nullptr, B->pts[B->cur].as<double2>(),
                       B->npts, B->A, B->img.as<unsigned int>());
    HIP_TRY(hipGetLastError());
    B->have_density = true;
    B->have_field = false;
    return NABO_OK;
}

int bundle_field(nabo_bundle *B, double b)
{
    const int R = bundle_radius(b);
    std::vector<double> w((size_t)2 * R + 1);
    bundle_weights(b, R, w.data());
    const size_t px = (size_t)(B->A + 1) * (B->A + 1);
    int rc = B->w.reserve(w.size() * 8);
    if (rc || (rc = B->tmp.reserve(px * 8)) || (rc = B->blur.reserve(px * 8)) || (rc = B->field.reserve(px * 16))) return rc;
    HIP_TRY(hipMemcpy(B->w.p, w.data(), w.size() * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(&bundle_sc(B)->mx, 0, 8, nullptr));
    const unsigned grid = nabo::bundle_grid((int64_t)px, nabo::BND_THREADS);
    hipLaunchKernelGGL(nabo::bundle_blur_kernel<unsigned int>, dim3(grid), dim3(nabo::BND_THREADS), 0, nullptr, B->img.as<unsigned int>(),
                       B->tmp.as<double>(), B->A, R, B->w.as<double>(), 0, (unsigned long long *)nullptr);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(nabo::bundle_blur_kernel<double>, dim3(grid), dim3(nabo::BND_THREADS), 0, nullptr, B->tmp.as<double>(),
                       B->blur.as<double>(), B->A, R, B->w.as<double>(), 1, &bundle_sc(B)->mx);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(nabo::bundle_field_kernel, dim3(grid), dim3(nabo::BND_THREADS), 0, nullptr, B->blur.as<double>(), B->A,
                       &bundle_sc(B)->mx, B->field.as<double2>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(nullptr));   // (w is host memory of this call)
    B->have_field = true;
    return NABO_OK;
}

int bundle_smooth(nabo_bundle *B, int64_t passes)
{
    if (passes == 0) return NABO_OK;
    int rc = B->ends.reserve((size_t)B->npts);
    if (rc || (rc = bundle_room(B, 1 - B->cur, B->npts, 0))) return rc;
    HIP_TRY(hipMemsetAsync(B->ends.p, 0, (size_t)B->npts, nullptr));
    hipLaunchKernelGGL(nabo::bundle_ends_kernel, dim3(nabo::bundle_grid(B->E, nabo::BND_THREADS)), dim3(nabo::BND_THREADS), 0, nullptr,
                       B->off[B->cur].as<int64_t>(), B->E, B->ends.as<uint8_t>());
    HIP_TRY(hipGetLastError());
    const double keep = 1.0 - B->tension, half = B->tension * 0.5;
    int in = B->cur;
    for (int64_t k = 0; k < passes; ++k) {
        hipLaunchKernelGGL(nabo::bundle_smooth_kernel, dim3(nabo::bundle_grid(B->npts, nabo::BND_THREADS)), dim3(nabo::BND_THREADS), 0, nullptr,
                           B->pts[in].as<double2>(), B->pts[1 - in].as<double2>(), B->ends.as<uint8_t>(), B->npts, keep, half);
        HIP_TRY(hipGetLastError());
        in = 1 - in;
    }
    HIP_TRY(hipStreamSynchronize(nullptr));
    if (in != B->cur) {   // the points moved to the other buffer: its offsets are this one's
        HIP_TRY(hipMemcpy(B->off[in].p, B->off[B->cur].p, (size_t)(B->E + 1) * 8, hipMemcpyDeviceToDevice));
        B->cur = in;
    }
    B->have_density = false;
    return NABO_OK;
}

int bundle_create(nabo_bundle *B, int64_t n, const double *x, const double *y, int64_t E, const int64_t *src, const int64_t *dst)
{
    B->n = n;
    B->E = E;
    const double *c[2] = {x, y};
    for (int a = 0; a < 2; ++a) {
        double mn = c[a][0], mx = c[a][0];
        for (int64_t i = 1; i < n; ++i) {
            mn = std::min(mn, c[a][i]);
            mx = std::max(mx, c[a][i]);
        }
        B->lo[a] = mn;
        B->span[a] = mx - mn;
    }
    std::vector<double> pts((size_t)E * 4);
    std::vector<int64_t> off((size_t)E + 1);
    for (int64_t e = 0; e <= E; ++e) off[(size_t)e] = 2 * e;
    for (int64_t e = 0; e < E; ++e) {
        const int64_t ends[2] = {src[e], dst[e]};
        for (int k = 0; k < 2; ++k)
            for (int a = 0; a < 2; ++a)
                pts[(size_t)e * 4 + 2 * k + a] = B->span[a] == 0.0 ? 0.0 : (c[a][ends[k]] - B->lo[a]) / B->span[a];
    }
    for (int k = 0; k < 2; ++k) HIP_TRY(B->off[k].alloc((size_t)(E + 1) * 8));
    HIP_TRY(B->sc.alloc(sizeof(BundleScalars)));
    HIP_TRY(hipMemset(B->sc.p, 0, sizeof(BundleScalars)));
    for (hipEvent_t &e : B->ev) HIP_TRY(hipEventCreate(&e));
    int rc = bundle_room(B, 0, 2 * E, 0);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(B->off[0].p, off.data(), off.size() * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(B->pts[0].p, pts.data(), pts.size() * 8, hipMemcpyHostToDevice));
    B->npts = 2 * E;
    return NABO_OK;
}

int bundle_enter(nabo_bundle *B)
{
    if (!B) return nabo::api_fail(NABO_E_INVALID, "bundle is NULL");
    return nabo::use_device(B->device);
}

}  // namespace

nabo::BundleView nabo::bundle_view(const nabo_bundle *B)
{
    return {B->device, B->E, B->npts, B->off[B->cur].as<int64_t>(), B->pts[B->cur].as<double>(),
            {B->lo[0], B->lo[1]}, {B->span[0], B->span[1]}};
}

extern "C" {

int nabo_bundle_geometry(int32_t *p_max, int32_t *short_group, int32_t *short_cap, int32_t *long_group)
{
    if (p_max) *p_max = nabo::BND_PMAX;
    if (short_group) *short_group = nabo::BND_SHORT_G;
    if (short_cap) *short_cap = nabo::BND_SHORT_CAP;
    if (long_group) *long_group = nabo::BND_LONG_G;
    return NABO_OK;
}

int nabo_bundle_blur_weights(double b, int32_t *R, double *w, int64_t cap)
{
    if (!(b >= 0.5 && b <= 16384.0)) return nabo::api_fail(NABO_E_INVALID, "b=%g must be in [0.5, 16384]", b);
    const int r = bundle_radius(b);
    if (R) *R = r;
    if (w) {
        if (cap < 2 * (int64_t)r + 1) return nabo::api_fail(NABO_E_INVALID, "w holds %lld weights, %d are needed", (long long)cap, 2 * r + 1);
        bundle_weights(b, r, w);
    }
    return NABO_OK;
}

int nabo_bundle_create(nabo_bundle **out, int32_t device, int64_t n, const double *x, const double *y, int64_t n_edges,
                       const int64_t *src, const int64_t *dst)
{
    if (!out) return nabo::api_fail(NABO_E_INVALID, "out is NULL");
    *out = nullptr;
    if (n < 1 || n_edges < 1) return nabo::api_fail(NABO_E_INVALID, "n=%lld and n_edges=%lld must be at least 1", (long long)n, (long long)n_edges);
    if (!x || !y || !src || !dst) return nabo::api_fail(NABO_E_INVALID, "x, y, src or dst is NULL");
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(x[i]) || !std::isfinite(y[i])) return nabo::api_fail(NABO_E_INVALID, "the position of node %lld is not finite", (long long)i);
    for (int64_t e = 0; e < n_edges; ++e)
        if (src[e] < 0 || src[e] >= n || dst[e] < 0 || dst[e] >= n)
            return nabo::api_fail(NABO_E_INVALID, "edge %lld = (%lld, %lld) names a node outside [0, %lld)", (long long)e, (long long)src[e],
                                  (long long)dst[e], (long long)n);
    int rc = nabo::use_device(device);
    if (rc) return rc;
    return nabo::create_handle(out, device, "nabo_bundle_create", [&](nabo_bundle *B) { return bundle_create(B, n, x, y, n_edges, src, dst); });
}

void nabo_bundle_destroy(nabo_bundle *B)
{
    if (!B) return;
    (void)hipSetDevice(B->device);
    delete B;
}

int nabo_bundle_set_params(nabo_bundle *B, double initial_bandwidth, double decay, int32_t iterations, int32_t accuracy,
                           int32_t advect_iterations, int32_t resample_every, double min_segment_length,
                           double max_segment_length, double tension, int32_t smooth_passes, int64_t batch_size)
{
    if (!B) return nabo::api_fail(NABO_E_INVALID, "bundle is NULL");
    (void)batch_size;
    if (!std::isfinite(initial_bandwidth) || initial_bandwidth <= 0.0) return nabo::api_fail(NABO_E_INVALID, "initial_bandwidth must be finite and > 0");
    if (!(decay > 0.0 && decay <= 1.0)) return nabo::api_fail(NABO_E_INVALID, "decay=%g must be in (0, 1]", decay);
    if (accuracy < 2 || accuracy > 4096) return nabo::api_fail(NABO_E_INVALID, "accuracy=%d must be in [2, 4096]", accuracy);
    if (iterations < 0 || advect_iterations < 0 || smooth_passes < 0 || resample_every < 1)
        return nabo::api_fail(NABO_E_INVALID, "iterations, advect_iterations and smooth_passes must be >= 0, resample_every >= 1");
    if (!std::isfinite(max_segment_length) || !(min_segment_length > 0.0 && min_segment_length <= max_segment_length))
        return nabo::api_fail(NABO_E_INVALID, "segment lengths must be finite with 0 < min <= max");
    if (!(tension >= 0.0 && tension <= 1.0)) return nabo::api_fail(NABO_E_INVALID, "tension=%g must be in [0, 1]", tension);
    if (accuracy != B->A) B->have_density = B->have_field = false;
    B->initial_bandwidth = initial_bandwidth;
    B->decay = decay;
    B->iterations = iterations;
    B->A = accuracy;
    B->advect_iterations = advect_iterations;
    B->resample_every = resample_every;
    B->min_seg = min_segment_length;
    B->max_seg = max_segment_length;
    B->tension = tension;
    B->smooth_passes = smooth_passes;
    return NABO_OK;
}

int nabo_bundle_set_option(nabo_bundle *B, const char *name, int64_t value)
{
    if (!B || !name) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    if (strcmp(name, "chunk_edges") != 0) return nabo::api_fail(NABO_E_INVALID, "unknown bundle option %s", name);
    if (value < 1 || value > ((int64_t)1 << 22)) return nabo::api_fail(NABO_E_INVALID, "chunk_edges=%lld must be in [1, 2^22]", (long long)value);
    B->chunk = value;
    return NABO_OK;
}

int nabo_bundle_get_points(nabo_bundle *B, int64_t *n_points, int64_t *offsets, double *points)
{
    int rc = bundle_enter(B);
    if (rc) return rc;
    if (n_points) *n_points = B->npts;
    if (offsets) HIP_TRY(hipMemcpy(offsets, B->off[B->cur].p, (size_t)(B->E + 1) * 8, hipMemcpyDeviceToHost));
    if (points) HIP_TRY(hipMemcpy(points, B->pts[B->cur].p, (size_t)B->npts * 16, hipMemcpyDeviceToHost));
    return NABO_OK;
}

int nabo_bundle_set_points(nabo_bundle *B, const int64_t *offsets, const double *points)
{
    int rc = bundle_enter(B);
    if (rc) return rc;
    if (!offsets || !points) return nabo::api_fail(NABO_E_INVALID, "offsets or points is NULL");
    if (offsets[0] != 0) return nabo::api_fail(NABO_E_INVALID, "offsets[0] = %lld, must be 0", (long long)offsets[0]);
    for (int64_t e = 0; e < B->E; ++e) {
        const int64_t p = offsets[e + 1] - offsets[e];
        if (p < 2 || p > nabo::BND_IN_MAX)
            return nabo::api_fail(NABO_E_INVALID, "edge %lld has %lld points, must be 2 .. %d", (long long)e, (long long)p, nabo::BND_IN_MAX);
    }
    const int64_t np = offsets[B->E];
    for (int64_t i = 0; i < 2 * np; ++i)
        if (!(points[i] >= 0.0 && points[i] <= 1.0)) return nabo::api_fail(NABO_E_INVALID, "coordinate %lld = %g is not in [0, 1]", (long long)i, points[i]);
    if ((rc = bundle_room(B, B->cur, np, 0))) return rc;
    HIP_TRY(hipMemcpy(B->off[B->cur].p, offsets, (size_t)(B->E + 1) * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(B->pts[B->cur].p, points, (size_t)np * 16, hipMemcpyHostToDevice));
    B->npts = np;
    B->have_density = false;
    return NABO_OK;
}

int nabo_bundle_resample(nabo_bundle *B)
{
    int rc = bundle_enter(B);
    return rc ? rc : bundle_round(B, 0);
}

int nabo_bundle_density(nabo_bundle *B, uint32_t *image)
{
    int rc = bundle_enter(B);
    if (rc || (rc = bundle_density(B))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    if (image) HIP_TRY(hipMemcpy(image, B->img.p, (size_t)(B->A + 1) * (B->A + 1) * 4, hipMemcpyDeviceToHost));
    return NABO_OK;
}

int nabo_bundle_field(nabo_bundle *B, double b, double *blurred, double *gx, double *gy)
{
    int rc = bundle_enter(B);
    if (rc) return rc;
    if (!(b >= 0.5 && b <= 16384.0)) return nabo::api_fail(NABO_E_INVALID, "b=%g must be in [0.5, 16384]", b);
    if (!B->have_density) return nabo::api_fail(NABO_E_INVALID, "no density of the present points: call nabo_bundle_density first");
    if ((rc = bundle_field(B, b))) return rc;
    const size_t px = (size_t)(B->A + 1) * (B->A + 1);
    if (blurred) HIP_TRY(hipMemcpy(blurred, B->blur.p, px * 8, hipMemcpyDeviceToHost));
    if (gx || gy) {
        std::vector<double> f(px * 2);
        HIP_TRY(hipMemcpy(f.data(), B->field.p, px * 16, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < px; ++i) {
            if (gx) gx[i] = f[2 * i];
            if (gy) gy[i] = f[2 * i + 1];
        }
    }
    return NABO_OK;
}

int nabo_bundle_advect(nabo_bundle *B, int64_t n_steps)
{
    int rc = bundle_enter(B);
    if (rc) return rc;
    if (n_steps < 1 || n_steps > 1000000) return nabo::api_fail(NABO_E_INVALID, "n_steps=%lld must be in [1, 10^6]", (long long)n_steps);
    if (!B->have_field) return nabo::api_fail(NABO_E_INVALID, "no field: call nabo_bundle_density and nabo_bundle_field first");
    return bundle_round(B, (int)n_steps);
}

int nabo_bundle_smooth(nabo_bundle *B, int64_t passes)
{
    int rc = bundle_enter(B);
    if (rc) return rc;
    if (passes < 0) return nabo::api_fail(NABO_E_INVALID, "passes=%lld is negative", (long long)passes);
    return bundle_smooth(B, passes);
}

int nabo_bundle_run(nabo_bundle *B)
{
    int rc = bundle_enter(B);
    if (rc) return rc;
    for (double &m : B->ms) m = 0;
    nabo::PhaseTimer T{B->ev, B->ms, BND_MS_TOTAL};
    if ((rc = T.start()) || (rc = bundle_round(B, 0)) || (rc = T.stop(BND_MS_RESAMPLE))) return rc;
    double d = B->decay;
    for (int i = 1; i <= B->iterations; ++i, d = d * B->decay) {
        const double b = (B->initial_bandwidth * d) * (double)B->A;
        if (b < 2.0) break;
        if (b > 16384.0) return nabo::api_fail(NABO_E_INVALID, "a bandwidth of %g pixels is more than 16384", b);
        if ((rc = T.start()) || (rc = bundle_density(B)) || (rc = T.stop(BND_MS_DENSITY))) return rc;
        if ((rc = T.start()) || (rc = bundle_field(B, b)) || (rc = T.stop(BND_MS_FIELD))) return rc;
        if (B->advect_iterations == 0) continue;
        if ((rc = T.start()) || (rc = bundle_round(B, B->advect_iterations)) || (rc = T.stop(BND_MS_ADVECT))) return rc;
    }
    if ((rc = T.start()) || (rc = bundle_smooth(B, B->smooth_passes)) || (rc = T.stop(BND_MS_SMOOTH))) return rc;
    return NABO_OK;
}

int nabo_bundle_result(nabo_bundle *B, int64_t *offsets, double *points)
{
    int rc = bundle_enter(B);
    if (rc) return rc;
    std::vector<int64_t> off((size_t)B->E + 1);
    HIP_TRY(hipMemcpy(off.data(), B->off[B->cur].p, off.size() * 8, hipMemcpyDeviceToHost));
    if (offsets) memcpy(offsets, off.data(), off.size() * 8);
    if (!points) return NABO_OK;
    std::vector<double> q((size_t)B->npts * 2);
    HIP_TRY(hipMemcpy(q.data(), B->pts[B->cur].p, q.size() * 8, hipMemcpyDeviceToHost));
    double *o = points;
    for (int64_t e = 0; e < B->E; ++e) {
        for (int64_t i = off[(size_t)e]; i < off[(size_t)e + 1]; ++i)
            for (int a = 0; a < 2; ++a) *o++ = q[(size_t)i * 2 + a] * B->span[a] + B->lo[a];
        *o++ = NAN;
        *o++ = NAN;
    }
    return NABO_OK;
}

int nabo_bundle_last_ms(nabo_bundle *B, double ms[6])
{
    if (!B || !ms) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    for (int i = 0; i < 6; ++i) ms[i] = B->ms[i];
    return NABO_OK;
}

}  // extern "C"
