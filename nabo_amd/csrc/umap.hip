// UMAP embedding of cells: smooth k-NN distances, the fuzzy graph and synchronous optimisation epochs
// (include/nabo_umap.h is the contract; nabo/_umap.py:7-39 make_umap is what it replaces).
//
// Graph build, once per set of lists.  A group of W lanes (W the power of two >= k, at least 8) holds one row of the
// lists in registers, one entry per lane: the row sum and rho, then the 64-step search for sigma, every sum a butterfly
// over the group (the header's TREE).  The memberships a[i][t] are stored once, so that both ends of a pair read the
// same bits.  The union writes two slots per list entry -- the arc (i -> j), and (j -> i) when row j does not list i --
// as a 64-bit key (row << 32 | column) with its weight; pruned and unused slots get the key of a row past the last.
// One radix sort of the keys orders every row by column, and the row pointer is read off the sorted keys.  No slot is
// placed by an atomic: the only atomic is the maximum of the weights, whose result does not depend on the order.
//
// Epoch, the hot path.  UM_GROUP lanes share a node and stride over its row; a lane that meets a firing arc issues the
// gather of y_j together with the arc's schedule, then draws its negative samples UM_BATCH at a time: the UM_BATCH
// indices are hashed and their positions gathered before the first is used.  Each lane sums in its own fixed order, the
// lanes are added by a butterfly, and lane 0 moves the node into the other position buffer.  No atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

#include "../../include/nabo_umap.h"
#include "host_common.h"
#include "umap_common.h"

namespace nabo {

constexpr int UM_THREADS = 256;
constexpr int UM_GROUP = 16;    // lanes per node of the epoch kernel: part of the definition (the order of a node's sum)
constexpr int UM_BATCH = 4;     // negative samples whose gathers are in flight together

// rowsum[i] = TREE(d), rho[i] = the smallest positive entry
template <int W>
__global__ __launch_bounds__(UM_THREADS) void umap_rowsum_kernel(const double *__restrict__ dist, int64_t n, int k,
                                                                 double *__restrict__ rowsum, double *__restrict__ rho)
{
    const int64_t i = ((int64_t)blockIdx.x * UM_THREADS + threadIdx.x) / W;
    const int t = threadIdx.x % W;
    const bool have = i < n && t < k;
    const double d = have ? dist[i * k + t] : 0.0;
    const double s = umap_tree<W>(d);
    double r = have && d > 0.0 ? d : std::numeric_limits<double>::infinity();
#pragma unroll
    for (int m = 1; m < W; m <<= 1) r = fmin(r, __shfl_xor(r, m, W));
    if (i < n && t == 0) {
        rowsum[i] = s;
        rho[i] = std::isinf(r) ? 0.0 : r;
    }
}

// total[0] = the row sums in 256 strided accumulators, then halved
__global__ __launch_bounds__(UM_THREADS) void umap_total_kernel(const double *__restrict__ rowsum, int64_t n, double *__restrict__ total)
{
    __shared__ double s[UM_THREADS];
    const int t = threadIdx.x;
    double acc = 0.0;
    for (int64_t i = t; i < n; i += UM_THREADS) acc += rowsum[i];
    s[t] = acc;
    __syncthreads();
    for (int h = UM_THREADS / 2; h > 0; h >>= 1) {
        if (t < h) s[t] += s[t + h];
        __syncthreads();
    }
    if (t == 0) total[0] = s[0];
}

template <int W>
__global__ __launch_bounds__(UM_THREADS) void umap_smooth_kernel(const double *__restrict__ dist, int64_t n, int k, double target,
                                                                 const double *__restrict__ rowsum, const double *__restrict__ rho,
                                                                 const double *__restrict__ total, double *__restrict__ sigma)
{
    const int64_t i = ((int64_t)blockIdx.x * UM_THREADS + threadIdx.x) / W;
    const int t = threadIdx.x % W;
    const bool live = i < n;
    const bool term = live && t >= 1 && t < k;
    const double r = live ? rho[i] : 0.0;
    const double x = term ? dist[i * k + t] - r : 0.0;
    double lo = 0.0, hi = std::numeric_limits<double>::infinity(), mid = 1.0;
    bool done = !live;
    for (int step = 0; step < 64; ++step) {
        double v = 0.0;
        if (term) v = x > 0.0 ? exp(-(x / mid)) : 1.0;
        const double p = umap_tree<W>(v);
        if (!done) {
            if (fabs(p - target) < 1e-5)
                done = true;
            else if (p > target) {
                hi = mid;
                mid = (lo + hi) / 2.0;
            } else {
                lo = mid;
                if (std::isinf(hi)) mid = mid * 2.0;
                else mid = (lo + hi) / 2.0;
            }
        }
        if (__all(done)) break;
    }
    if (live && t == 0) {
        const double mean = r > 0.0 ? rowsum[i] / (double)k : total[0] / ((double)n * (double)k);
        sigma[i] = fmax(mid, 1e-3 * mean);
    }
}

__global__ __launch_bounds__(UM_THREADS) void umap_member_kernel(const int64_t *__restrict__ idx, const double *__restrict__ dist,
                                                                 int64_t n, int k, const double *__restrict__ rho,
                                                                 const double *__restrict__ sigma, double *__restrict__ a)
{
    const int64_t q = (int64_t)blockIdx.x * UM_THREADS + threadIdx.x;
    if (q >= n * k) return;
    const int64_t i = q / k;
    const double x = dist[q] - rho[i], s = sigma[i];
    double v;
    if (idx[q] == i) v = 0.0;
    else if (x <= 0.0 || s == 0.0) v = 1.0;
    else v = exp(-(x / s));
    a[q] = v;
}

// two slots per list entry: [2q] the arc (i -> j), [2q + 1] the arc (j -> i) when row j does not list i
__global__ __launch_bounds__(UM_THREADS) void umap_union_kernel(const int64_t *__restrict__ idx, const double *__restrict__ a, int64_t n,
                                                                int k, uint64_t *__restrict__ keys, double *__restrict__ w,
                                                                unsigned long long *__restrict__ wmax_bits)
{
    const int64_t q = (int64_t)blockIdx.x * UM_THREADS + threadIdx.x;
    if (q >= n * k) return;
    const uint64_t none = (uint64_t)n << 32;
    const int64_t i = q / k, j = idx[q];
    uint64_t kf = none, kr = none;
    double wv = 0.0;
    if (j != i) {
        const double aij = a[q];
        double aji = 0.0;
        bool found = false;
        const int64_t *row = idx + j * k;
        for (int s = 0; s < k; ++s)
            if (row[s] == i) {
                found = true;
                aji = a[j * k + s];
            }
        wv = (aij + aji) - aij * aji;
        kf = ((uint64_t)i << 32) | (uint64_t)j;
        if (!found) kr = ((uint64_t)j << 32) | (uint64_t)i;
        atomicMax(wmax_bits, (unsigned long long)__double_as_longlong(wv));   // w >= 0: its bits order as its value
    }
    keys[2 * q] = kf;
    keys[2 * q + 1] = kr;
    w[2 * q] = wv;
    w[2 * q + 1] = wv;
}

__global__ __launch_bounds__(UM_THREADS) void umap_prune_kernel(uint64_t *__restrict__ keys, const double *__restrict__ w, int64_t n_slots,
                                                                int64_t n, const double *__restrict__ wmax, double n_epochs)
{
    const int64_t q = (int64_t)blockIdx.x * UM_THREADS + threadIdx.x;
    if (q >= n_slots) return;
    if (w[q] < wmax[0] / n_epochs) keys[q] = (uint64_t)n << 32;
}

// the arcs of the pruned CSR and the first state of their schedule
__global__ __launch_bounds__(UM_THREADS) void umap_arcs_kernel(const uint64_t *__restrict__ keys, const double *__restrict__ w, int64_t n_arcs,
                                                               const double *__restrict__ wmax, double nsr, int32_t *__restrict__ nbr,
                                                               double *__restrict__ eps, double *__restrict__ epn, double *__restrict__ next,
                                                               double *__restrict__ nneg)
{
    const int64_t e = (int64_t)blockIdx.x * UM_THREADS + threadIdx.x;
    if (e >= n_arcs) return;
    const double s = wmax[0] / w[e], sn = s / nsr;
    if (nbr) nbr[e] = (int32_t)(keys[e] & 0xFFFFFFFFull);
    eps[e] = s;
    epn[e] = sn;
    next[e] = s;
    nneg[e] = sn;
}

template <int DIMS>
__global__ __launch_bounds__(UM_THREADS) void umap_epoch_kernel(int64_t n, const int64_t *__restrict__ ptr, const int32_t *__restrict__ nbr,
                                                                const double *__restrict__ eps, const double *__restrict__ epn,
                                                                double *__restrict__ next, double *__restrict__ nneg,
                                                                const double *__restrict__ y, double *__restrict__ ynew, UmapEpoch P,
                                                                int32_t *__restrict__ n_attr, int32_t *__restrict__ n_neg,
                                                                uint64_t *__restrict__ idx_sum)
{
    const int64_t i = ((int64_t)blockIdx.x * UM_THREADS + threadIdx.x) / UM_GROUP;
    const int l = threadIdx.x % UM_GROUP;
    double yi[DIMS], acc[DIMS];
    int na = 0, nn = 0;
    uint64_t ks = 0;
#pragma unroll
    for (int c = 0; c < DIMS; ++c) yi[c] = acc[c] = 0.0;
    if (i < n) {
#pragma unroll
        for (int c = 0; c < DIMS; ++c) yi[c] = y[i * DIMS + c];
        const int64_t e1 = ptr[i + 1];
        for (int64_t e = ptr[i] + l; e < e1; e += UM_GROUP) {
            const double nx = next[e];
            if (!(nx <= P.t)) continue;
            // (i) the head's position and the arc's schedule, all loads issued before the first use
            const int64_t j = nbr[e];
            const double es = eps[e], en = epn[e], ng = nneg[e];
            double yj[DIMS];
#pragma unroll
            for (int c = 0; c < DIMS; ++c) yj[c] = y[j * DIMS + c];
            const int64_t m = (int64_t)((P.t - ng) / en);
            const uint64_t se = umap_mix(P.s_t + UM_GOLD * ((uint64_t)e + 1));
            {
                double D[DIMS], d2 = 0.0;
#pragma unroll
                for (int c = 0; c < DIMS; ++c) {
                    D[c] = yi[c] - yj[c];
                    d2 += D[c] * D[c];
                }
                const double cf = d2 > 0.0 ? (P.ca * pow(d2, P.b - 1.0)) / (P.a * pow(d2, P.b) + 1.0) : 0.0;
#pragma unroll
                for (int c = 0; c < DIMS; ++c) acc[c] += 2.0 * umap_clip(cf * D[c]);
                ++na;
            }
            next[e] = nx + es;
            // (ii) negative samples, UM_BATCH gathers in flight
            for (int64_t p0 = 0; p0 < m; p0 += UM_BATCH) {
                int64_t kk[UM_BATCH];
                double yk[UM_BATCH][DIMS];
#pragma unroll
                for (int q = 0; q < UM_BATCH; ++q) {
                    const uint64_t z = umap_mix(se + UM_GOLD * ((uint64_t)(p0 + q) + 1));
                    kk[q] = p0 + q < m ? (int64_t)(((z >> 32) * (uint64_t)n) >> 32) : i;
#pragma unroll
                    for (int c = 0; c < DIMS; ++c) yk[q][c] = y[kk[q] * DIMS + c];
                }
#pragma unroll
                for (int q = 0; q < UM_BATCH; ++q) {
                    if (p0 + q < m) {
                        ++nn;
                        ks += (uint64_t)kk[q];
                    }
                    if (kk[q] == i) continue;
                    double D[DIMS], d2 = 0.0;
#pragma unroll
                    for (int c = 0; c < DIMS; ++c) {
                        D[c] = yi[c] - yk[q][c];
                        d2 += D[c] * D[c];
                    }
                    const double cf = d2 > 0.0 ? P.cr / ((0.001 + d2) * (P.a * pow(d2, P.b) + 1.0)) : 0.0;
#pragma unroll
                    for (int c = 0; c < DIMS; ++c) acc[c] += umap_clip(cf * D[c]);
                }
            }
            nneg[e] = ng + (double)m * en;
        }
    }
#pragma unroll
    for (int c = 0; c < DIMS; ++c) acc[c] = umap_tree<UM_GROUP>(acc[c]);
#pragma unroll
    for (int m = 1; m < UM_GROUP; m <<= 1) {
        na += __shfl_xor(na, m, UM_GROUP);
        nn += __shfl_xor(nn, m, UM_GROUP);
        ks += (uint64_t)__shfl_xor((unsigned long long)ks, m, UM_GROUP);
    }
    if (i < n && l == 0) {
#pragma unroll
        for (int c = 0; c < DIMS; ++c) ynew[i * DIMS + c] = yi[c] + P.alpha * acc[c];
        n_attr[i] = na;
        n_neg[i] = nn;
        idx_sum[i] = ks;
    }
}

int umap_group() { return UM_GROUP; }

static int umap_width(int k) { return k <= 8 ? 8 : k <= 16 ? 16 : k <= 32 ? 32 : 64; }

hipError_t umap_smooth_launch(const double *dist, int64_t n, int k, double target, double *rowsum, double *rho, double *total,
                              double *sigma, hipStream_t st)
{
    const int W = umap_width(k);
    const unsigned grid = (unsigned)((n * W + UM_THREADS - 1) / UM_THREADS);
#define UMAP_W(WW)                                                                                                            \
    hipLaunchKernelGGL(umap_rowsum_kernel<WW>, dim3(grid), dim3(UM_THREADS), 0, st, dist, n, k, rowsum, rho);                \
    hipLaunchKernelGGL(umap_total_kernel, dim3(1), dim3(UM_THREADS), 0, st, rowsum, n, total);                                \
    hipLaunchKernelGGL(umap_smooth_kernel<WW>, dim3(grid), dim3(UM_THREADS), 0, st, dist, n, k, target, rowsum, rho, total, sigma)
    if (W == 8) { UMAP_W(8); }
    else if (W == 16) { UMAP_W(16); }
    else if (W == 32) { UMAP_W(32); }
    else { UMAP_W(64); }
#undef UMAP_W
    return hipGetLastError();
}

hipError_t umap_sort_temp_bytes(int64_t n_slots, int64_t n, size_t *bytes)
{
    *bytes = 0;
    return rocprim::radix_sort_pairs(nullptr, *bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const double *)nullptr,
                                     (double *)nullptr, (size_t)n_slots, 0u, key_sort_bits(n), (hipStream_t) nullptr);
}

hipError_t umap_graph_launch(const int64_t *idx, const double *dist, int64_t n, int k, const double *rho, const double *sigma,
                             double n_epochs, double *a, uint64_t *keys_a, double *w_a, uint64_t *keys_b, double *w_b, void *temp,
                             size_t temp_bytes, double *wmax, int64_t *ptr, hipStream_t st)
{
    const int64_t nk = n * k, n_slots = 2 * nk;
    const unsigned g1 = (unsigned)((nk + UM_THREADS - 1) / UM_THREADS), g2 = (unsigned)((n_slots + UM_THREADS - 1) / UM_THREADS);
    hipError_t e = hipMemsetAsync(wmax, 0, 8, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(umap_member_kernel, dim3(g1), dim3(UM_THREADS), 0, st, idx, dist, n, k, rho, sigma, a);
    hipLaunchKernelGGL(umap_union_kernel, dim3(g1), dim3(UM_THREADS), 0, st, idx, a, n, k, keys_a, w_a,
                       reinterpret_cast<unsigned long long *>(wmax));
    hipLaunchKernelGGL(umap_prune_kernel, dim3(g2), dim3(UM_THREADS), 0, st, keys_a, w_a, n_slots, n, wmax, n_epochs);
    e = rocprim::radix_sort_pairs(temp, temp_bytes, (const uint64_t *)keys_a, keys_b, (const double *)w_a, w_b, (size_t)n_slots, 0u,
                                  key_sort_bits(n), st);
    if (e != hipSuccess) return e;
    return key_rowptr_launch(keys_b, n_slots, n, ptr, st);   // unused slots carry row n
}

hipError_t umap_arcs_launch(const uint64_t *keys, const double *w, int64_t n_arcs, const double *wmax, double nsr, int32_t *nbr,
                            double *eps, double *epn, double *next, double *nneg, hipStream_t st)
{
    if (n_arcs == 0) return hipSuccess;
    hipLaunchKernelGGL(umap_arcs_kernel, dim3((unsigned)((n_arcs + UM_THREADS - 1) / UM_THREADS)), dim3(UM_THREADS), 0, st, keys, w,
                       n_arcs, wmax, nsr, nbr, eps, epn, next, nneg);
    return hipGetLastError();
}

hipError_t umap_epoch_launch(int dims, int64_t n, const int64_t *ptr, const int32_t *nbr, const double *eps, const double *epn,
                             double *next, double *nneg, const double *y, double *ynew, const UmapEpoch &P, int32_t *n_attr,
                             int32_t *n_neg, uint64_t *idx_sum, hipStream_t st)
{
    const unsigned grid = (unsigned)((n * UM_GROUP + UM_THREADS - 1) / UM_THREADS);
    if (dims == 2)
        hipLaunchKernelGGL(umap_epoch_kernel<2>, dim3(grid), dim3(UM_THREADS), 0, st, n, ptr, nbr, eps, epn, next, nneg, y, ynew, P,
                           n_attr, n_neg, idx_sum);
    else
        hipLaunchKernelGGL(umap_epoch_kernel<3>, dim3(grid), dim3(UM_THREADS), 0, st, n, ptr, nbr, eps, epn, next, nneg, y, ynew, P,
                           n_attr, n_neg, idx_sum);
    return hipGetLastError();
}

}  // namespace nabo

using nabo::DevBuf;

namespace {
constexpr int UM_TIMED = 16;   // epochs of a run that are timed one by one (its last ones)
}

struct nabo_umap {
    int device = 0, dims = 2, k = 0;
    int64_t n = 0, n_arcs = 0, n_epochs = 200, epoch = 0;
    int nsr = 5;
    double gamma = 1.0, a = 1.577, b = 0.895;
    uint64_t seed = 0;
    bool have_graph = false, ran = false;
    int cur = 0;   // which of y[2] holds the embedding
    DevBuf y[2], idx, dist, X, rowsum, total, rho, sigma, memb, keys_a, keys_b, w_a, w_b, temp, wmax, ptr, nbr, eps, epn, next, nneg,
        n_attr, n_neg, idx_sum;
    hipEvent_t ev[UM_TIMED + 1 + 4] = {};
    double ms[4] = {0, 0, 0, 0};
    int64_t n_timed = 0;
    ~nabo_umap()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

namespace {

// the arcs of the CSR in U->keys_b, U->w_b (E of them, wmax in U->wmax) and the first state of their schedule
int umap_arcs(nabo_umap *U, int64_t E)
{
    U->n_arcs = E;
    HIP_TRY(U->nbr.alloc((size_t)E * 4));
    for (DevBuf *b : {&U->eps, &U->epn, &U->next, &U->nneg}) HIP_TRY(b->alloc((size_t)E * 8));
    HIP_TRY(nabo::umap_arcs_launch(U->keys_b.as<uint64_t>(), U->w_b.as<double>(), E, U->wmax.as<double>(), (double)U->nsr,
                                   U->nbr.as<int32_t>(), U->eps.as<double>(), U->epn.as<double>(), U->next.as<double>(),
                                   U->nneg.as<double>(), nullptr));
    return NABO_OK;
}

// parts B and C from the lists in U->idx, U->dist (device), then the arcs and their schedule
int umap_build(nabo_umap *U, int k)
{
    const int64_t n = U->n, nk = n * k, n_slots = 2 * nk;
    hipStream_t st = nullptr;
    U->have_graph = false;
    U->k = k;
    for (DevBuf *b : {&U->rowsum, &U->rho, &U->sigma}) HIP_TRY(b->alloc((size_t)n * 8));
    HIP_TRY(U->total.alloc(8));
    HIP_TRY(U->wmax.alloc(8));
    HIP_TRY(U->memb.alloc((size_t)nk * 8));
    for (DevBuf *b : {&U->keys_a, &U->keys_b, &U->w_a, &U->w_b}) HIP_TRY(b->alloc((size_t)n_slots * 8));
    HIP_TRY(U->ptr.alloc(((size_t)n + 1) * 8));
    size_t tb = 0;
    HIP_TRY(nabo::umap_sort_temp_bytes(n_slots, n, &tb));
    HIP_TRY(U->temp.alloc(tb));
    hipEvent_t *ev = U->ev + UM_TIMED + 1;
    HIP_TRY(hipEventRecord(ev[0], st));
    HIP_TRY(nabo::umap_smooth_launch(U->dist.as<double>(), n, k, std::log2((double)k), U->rowsum.as<double>(), U->rho.as<double>(),
                                     U->total.as<double>(), U->sigma.as<double>(), st));
    HIP_TRY(nabo::umap_graph_launch(U->idx.as<int64_t>(), U->dist.as<double>(), n, k, U->rho.as<double>(), U->sigma.as<double>(),
                                    (double)U->n_epochs, U->memb.as<double>(), U->keys_a.as<uint64_t>(), U->w_a.as<double>(),
                                    U->keys_b.as<uint64_t>(), U->w_b.as<double>(), U->temp.p, tb, U->wmax.as<double>(),
                                    U->ptr.as<int64_t>(), st));
    HIP_TRY(hipStreamSynchronize(st));
    int64_t E = 0;
    HIP_TRY(hipMemcpy(&E, U->ptr.as<int64_t>() + n, 8, hipMemcpyDeviceToHost));
    if (E < 0 || E > n_slots) return nabo::api_fail(NABO_E_HIP, "the graph build returned %lld arcs for %lld slots", (long long)E, (long long)n_slots);
    int rc = umap_arcs(U, E);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(ev[1], st));
    HIP_TRY(hipStreamSynchronize(st));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
    U->ms[0] = ms;
    // the sort's scratch is not needed again; the sorted keys and weights stay (get_graph, rewind)
    U->keys_a.release();
    U->w_a.release();
    U->temp.release();
    U->memb.release();
    U->epoch = 0;
    U->have_graph = true;
    return NABO_OK;
}

int umap_rewind(nabo_umap *U)
{
    U->epoch = 0;
    if (!U->have_graph) return NABO_OK;
    HIP_TRY(nabo::umap_arcs_launch(U->keys_b.as<uint64_t>(), U->w_b.as<double>(), U->n_arcs, U->wmax.as<double>(), (double)U->nsr, nullptr,
                                   U->eps.as<double>(), U->epn.as<double>(), U->next.as<double>(), U->nneg.as<double>(), nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return NABO_OK;
}

int umap_check_k(const nabo_umap *U, int32_t k)
{
    if (k < 2 || k > NABO_MAX_K) return nabo::api_fail(NABO_E_INVALID, "k=%d must be in [2, %d]", (int)k, NABO_MAX_K);
    if (k >= U->n) return nabo::api_fail(NABO_E_INVALID, "k=%d must be below n=%lld", (int)k, (long long)U->n);
    return NABO_OK;
}

}  // namespace

extern "C" {

int nabo_umap_geometry(int32_t *group)
{
    if (group) *group = nabo::UM_GROUP;
    return NABO_OK;
}

int nabo_umap_create(nabo_umap **out, int32_t device, int64_t n, int32_t dims)
{
    if (!out) return nabo::api_fail(NABO_E_INVALID, "out is NULL");
    *out = nullptr;
    if (n < 3) return nabo::api_fail(NABO_E_INVALID, "n=%lld must be at least 3", (long long)n);
    if (n >= ((int64_t)1 << 31)) return nabo::api_fail(NABO_E_UNSUPPORTED, "n=%lld: the embedding takes fewer than 2^31 cells", (long long)n);
    if (dims != 2 && dims != 3) return nabo::api_fail(NABO_E_INVALID, "dims=%d must be 2 or 3", (int)dims);
    int rc = nabo::use_device(device);
    if (rc) return rc;
    nabo_umap *U = new nabo_umap;
    U->device = device;
    U->n = n;
    U->dims = dims;
    auto init = [&]() -> int {
        const size_t yb = (size_t)n * dims * 8;
        for (DevBuf &b : U->y) {
            HIP_TRY(b.alloc(yb));
            HIP_TRY(hipMemset(b.p, 0, yb));
        }
        HIP_TRY(U->n_attr.alloc((size_t)n * 4));
        HIP_TRY(U->n_neg.alloc((size_t)n * 4));
        HIP_TRY(U->idx_sum.alloc((size_t)n * 8));
        for (hipEvent_t &e : U->ev) HIP_TRY(hipEventCreate(&e));
        return NABO_OK;
    };
    rc = init();
    if (rc) {
        delete U;
        return rc;
    }
    *out = U;
    return NABO_OK;
}

void nabo_umap_destroy(nabo_umap *U)
{
    if (!U) return;
    (void)hipSetDevice(U->device);
    delete U;
}

int nabo_umap_set_params(nabo_umap *U, int64_t n_epochs, int32_t negative_sample_rate, double repulsion_strength, double a, double b,
                         uint64_t seed)
{
    if (!U) return nabo::api_fail(NABO_E_INVALID, "umap is NULL");
    if (n_epochs < 1) return nabo::api_fail(NABO_E_INVALID, "n_epochs=%lld must be at least 1", (long long)n_epochs);
    if (negative_sample_rate < 1) return nabo::api_fail(NABO_E_INVALID, "negative_sample_rate=%d must be at least 1", (int)negative_sample_rate);
    if (!std::isfinite(repulsion_strength) || !std::isfinite(a) || !std::isfinite(b) || !(a > 0.0) || !(b > 0.0))
        return nabo::api_fail(NABO_E_INVALID, "repulsion_strength, a and b must be finite, a and b positive");
    if (U->have_graph && n_epochs != U->n_epochs) U->have_graph = false;
    U->n_epochs = n_epochs;
    U->nsr = negative_sample_rate;
    U->gamma = repulsion_strength;
    U->a = a;
    U->b = b;
    U->seed = seed;
    if (!U->have_graph) {
        U->epoch = 0;
        return NABO_OK;
    }
    int rc = nabo::use_device(U->device);
    if (rc) return rc;
    return umap_rewind(U);
}

int nabo_umap_set_knn(nabo_umap *U, const int64_t *idx, const double *dist, int32_t k)
{
    if (!U || !idx || !dist) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    int rc = umap_check_k(U, k);
    if (rc) return rc;
    const int64_t n = U->n;
    for (int64_t i = 0; i < n; ++i)
        for (int t = 0; t < k; ++t) {
            const int64_t q = i * k + t;
            if (idx[q] < 0 || idx[q] >= n)
                return nabo::api_fail(NABO_E_INVALID, "idx[%lld][%d] = %lld is not a cell in [0, %lld)", (long long)i, t, (long long)idx[q], (long long)n);
            if (!std::isfinite(dist[q]) || dist[q] < 0.0 || (t > 0 && dist[q] < dist[q - 1]))
                return nabo::api_fail(NABO_E_INVALID, "dist[%lld][%d] is not finite, is negative or is below its predecessor", (long long)i, t);
        }
    rc = nabo::use_device(U->device);
    if (rc) return rc;
    const size_t nb = (size_t)n * k * 8;
    HIP_TRY(U->idx.alloc(nb));
    HIP_TRY(U->dist.alloc(nb));
    HIP_TRY(hipMemcpy(U->idx.p, idx, nb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(U->dist.p, dist, nb, hipMemcpyHostToDevice));
    U->ms[1] = 0;
    return umap_build(U, k);
}

int nabo_umap_fit_knn(nabo_umap *U, const double *X, int32_t g, int32_t k, int32_t metric, double dist_factor)
{
    if (!U || !X) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    int rc = umap_check_k(U, k);
    if (rc) return rc;
    if (g < 1) return nabo::api_fail(NABO_E_INVALID, "g=%d must be at least 1", (int)g);
    rc = nabo::use_device(U->device);
    if (rc) return rc;
    const int64_t n = U->n;
    nabo_index *ix = nullptr;
    rc = nabo_index_create(&ix, U->device, n, g, metric, dist_factor, 0);
    if (rc) return rc;
    auto query = [&]() -> int {
        HIP_TRY(U->X.alloc((size_t)n * g * 8));
        HIP_TRY(U->idx.alloc((size_t)n * k * 8));
        HIP_TRY(U->dist.alloc((size_t)n * k * 8));
        HIP_TRY(hipMemcpy(U->X.p, X, (size_t)n * g * 8, hipMemcpyHostToDevice));
        int r = nabo_index_set_ref(ix, U->X.as<double>(), 1, nullptr);
        if (r) return r;
        hipEvent_t *ev = U->ev + UM_TIMED + 1 + 2;
        HIP_TRY(hipEventRecord(ev[0], nullptr));
        r = nabo_index_query(ix, U->X.as<double>(), 1, n, k, 0, U->idx.as<int64_t>(), U->dist.as<double>(), 1);
        if (r) return r;
        HIP_TRY(hipEventRecord(ev[1], nullptr));
        HIP_TRY(hipDeviceSynchronize());
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
        U->ms[1] = ms;
        return NABO_OK;
    };
    rc = query();
    (void)nabo_index_destroy(ix);
    U->X.release();
    if (rc) return rc;
    return umap_build(U, k);
}

int nabo_umap_set_graph(nabo_umap *U, const int64_t *ptr, const int64_t *nbr, const double *w)
{
    if (!U || !ptr) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    const int64_t n = U->n;
    int rc = nabo::check_csr_ptr("ptr", "node", n, ptr);
    if (rc) return rc;
    const int64_t E = ptr[n];
    if (E < 1 || !nbr || !w) return nabo::api_fail(NABO_E_INVALID, "the graph has no arc, or nbr or w is NULL");
    std::vector<uint64_t> keys((size_t)E);
    double wmax = 0.0;
    for (int64_t i = 0; i < n; ++i)
        for (int64_t e = ptr[i]; e < ptr[i + 1]; ++e) {
            if (nbr[e] < 0 || nbr[e] >= n || nbr[e] == i)
                return nabo::api_fail(NABO_E_INVALID, "nbr[%lld] = %lld is not another node in [0, %lld)", (long long)e, (long long)nbr[e], (long long)n);
            if (!std::isfinite(w[e]) || !(w[e] > 0.0)) return nabo::api_fail(NABO_E_INVALID, "w[%lld] is not finite and positive", (long long)e);
            keys[(size_t)e] = ((uint64_t)i << 32) | (uint64_t)nbr[e];
            wmax = std::max(wmax, w[e]);
        }
    if ((rc = nabo::use_device(U->device))) return rc;
    U->have_graph = false;
    U->k = 0;
    for (DevBuf *b : {&U->rho, &U->sigma}) {
        HIP_TRY(b->alloc((size_t)n * 8));
        HIP_TRY(hipMemset(b->p, 0, (size_t)n * 8));
    }
    HIP_TRY(U->wmax.alloc(8));
    HIP_TRY(U->ptr.alloc(((size_t)n + 1) * 8));
    HIP_TRY(U->keys_b.alloc((size_t)E * 8));
    HIP_TRY(U->w_b.alloc((size_t)E * 8));
    HIP_TRY(hipMemcpy(U->wmax.p, &wmax, 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(U->ptr.p, ptr, ((size_t)n + 1) * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(U->keys_b.p, keys.data(), (size_t)E * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(U->w_b.p, w, (size_t)E * 8, hipMemcpyHostToDevice));
    rc = umap_arcs(U, E);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    U->ms[0] = U->ms[1] = 0;
    U->epoch = 0;
    U->have_graph = true;
    return NABO_OK;
}

int nabo_umap_graph_size(nabo_umap *U, int64_t *n_arcs, double *wmax)
{
    if (!U) return nabo::api_fail(NABO_E_INVALID, "umap is NULL");
    if (!U->have_graph) return nabo::api_fail(NABO_E_INVALID, "no graph: call nabo_umap_set_knn or nabo_umap_fit_knn first");
    int rc = nabo::use_device(U->device);
    if (rc) return rc;
    if (n_arcs) *n_arcs = U->n_arcs;
    if (wmax) HIP_TRY(hipMemcpy(wmax, U->wmax.p, 8, hipMemcpyDeviceToHost));
    return NABO_OK;
}

int nabo_umap_get_graph(nabo_umap *U, double *rho, double *sigma, int64_t *ptr, int64_t *nbr, double *w)
{
    if (!U) return nabo::api_fail(NABO_E_INVALID, "umap is NULL");
    if (!U->have_graph) return nabo::api_fail(NABO_E_INVALID, "no graph: call nabo_umap_set_knn or nabo_umap_fit_knn first");
    int rc = nabo::use_device(U->device);
    if (rc) return rc;
    const size_t nb = (size_t)U->n * 8, E = (size_t)U->n_arcs;
    if (rho) HIP_TRY(hipMemcpy(rho, U->rho.p, nb, hipMemcpyDeviceToHost));
    if (sigma) HIP_TRY(hipMemcpy(sigma, U->sigma.p, nb, hipMemcpyDeviceToHost));
    if (ptr) HIP_TRY(hipMemcpy(ptr, U->ptr.p, nb + 8, hipMemcpyDeviceToHost));
    if (nbr && E) {
        std::vector<int32_t> h(E);
        HIP_TRY(hipMemcpy(h.data(), U->nbr.p, E * 4, hipMemcpyDeviceToHost));
        for (size_t e = 0; e < E; ++e) nbr[e] = h[e];
    }
    if (w && E) HIP_TRY(hipMemcpy(w, U->w_b.p, E * 8, hipMemcpyDeviceToHost));
    return NABO_OK;
}

int nabo_umap_set_embedding(nabo_umap *U, const double *y)
{
    if (!U || !y) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    const size_t cnt = (size_t)U->n * U->dims;
    for (size_t q = 0; q < cnt; ++q)
        if (!std::isfinite(y[q])) return nabo::api_fail(NABO_E_INVALID, "y[%zu][%zu] is not finite", q / U->dims, q % U->dims);
    int rc = nabo::use_device(U->device);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(U->y[U->cur].p, y, cnt * 8, hipMemcpyHostToDevice));
    return NABO_OK;
}

int nabo_umap_get_embedding(nabo_umap *U, double *y)
{
    if (!U || !y) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    int rc = nabo::use_device(U->device);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(y, U->y[U->cur].p, (size_t)U->n * U->dims * 8, hipMemcpyDeviceToHost));
    return NABO_OK;
}

int nabo_umap_rewind(nabo_umap *U)
{
    if (!U) return nabo::api_fail(NABO_E_INVALID, "umap is NULL");
    int rc = nabo::use_device(U->device);
    if (rc) return rc;
    return umap_rewind(U);
}

int nabo_umap_run(nabo_umap *U, int64_t n_run, int64_t *done)
{
    if (!U) return nabo::api_fail(NABO_E_INVALID, "umap is NULL");
    if (n_run < 0) return nabo::api_fail(NABO_E_INVALID, "n_run=%lld is negative", (long long)n_run);
    if (done) *done = 0;
    if (!U->have_graph) return nabo::api_fail(NABO_E_INVALID, "no graph: call nabo_umap_set_knn or nabo_umap_fit_knn first");
    int rc = nabo::use_device(U->device);
    if (rc) return rc;
    n_run = std::min<int64_t>(n_run, U->n_epochs - U->epoch);
    U->ms[2] = U->ms[3] = 0;
    U->n_timed = 0;
    if (n_run <= 0) return NABO_OK;
    hipStream_t st = nullptr;
    nabo::UmapEpoch P;
    P.a = U->a;
    P.b = U->b;
    P.ca = (-2.0 * U->a) * U->b;
    P.cr = (2.0 * U->gamma) * U->b;
    const int64_t first_timed = n_run > UM_TIMED ? n_run - UM_TIMED : 0;
    hipEvent_t *run_ev = U->ev + UM_TIMED + 1;   // shared with the build's pair: a run never overlaps a build
    HIP_TRY(hipEventRecord(run_ev[0], st));
    for (int64_t it = 0; it < n_run; ++it) {
        const int64_t t = U->epoch;
        P.t = (double)t;
        P.alpha = 1.0 - (double)t / (double)U->n_epochs;
        P.s_t = nabo::umap_mix(U->seed + nabo::UM_GOLD * ((uint64_t)t + 1));
        if (it >= first_timed) HIP_TRY(hipEventRecord(U->ev[it - first_timed], st));
        HIP_TRY(nabo::umap_epoch_launch(U->dims, U->n, U->ptr.as<int64_t>(), U->nbr.as<int32_t>(), U->eps.as<double>(),
                                        U->epn.as<double>(), U->next.as<double>(), U->nneg.as<double>(), U->y[U->cur].as<double>(),
                                        U->y[U->cur ^ 1].as<double>(), P, U->n_attr.as<int32_t>(), U->n_neg.as<int32_t>(),
                                        U->idx_sum.as<uint64_t>(), st));
        U->cur ^= 1;
        U->epoch = t + 1;
    }
    HIP_TRY(hipEventRecord(U->ev[n_run - first_timed], st));
    HIP_TRY(hipEventRecord(run_ev[1], st));
    HIP_TRY(hipStreamSynchronize(st));
    U->ran = true;
    if (done) *done = n_run;
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, run_ev[0], run_ev[1]));
    U->ms[3] = ms;
    U->n_timed = n_run - first_timed;
    HIP_TRY(hipEventElapsedTime(&ms, U->ev[0], U->ev[U->n_timed]));
    U->ms[2] = ms / (double)U->n_timed;
    return NABO_OK;
}

int nabo_umap_last_epoch_counts(nabo_umap *U, int32_t *n_attr, int32_t *n_neg, uint64_t *idx_sum)
{
    if (!U) return nabo::api_fail(NABO_E_INVALID, "umap is NULL");
    if (!U->ran) return nabo::api_fail(NABO_E_INVALID, "no epoch has run on this embedding");
    int rc = nabo::use_device(U->device);
    if (rc) return rc;
    if (n_attr) HIP_TRY(hipMemcpy(n_attr, U->n_attr.p, (size_t)U->n * 4, hipMemcpyDeviceToHost));
    if (n_neg) HIP_TRY(hipMemcpy(n_neg, U->n_neg.p, (size_t)U->n * 4, hipMemcpyDeviceToHost));
    if (idx_sum) HIP_TRY(hipMemcpy(idx_sum, U->idx_sum.p, (size_t)U->n * 8, hipMemcpyDeviceToHost));
    return NABO_OK;
}

int nabo_umap_last_ms(nabo_umap *U, double ms[4], int64_t *n_timed)
{
    if (!U || !ms) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    for (int i = 0; i < 4; ++i) ms[i] = U->ms[i];
    if (n_timed) *n_timed = U->n_timed;
    return NABO_OK;
}

}  // extern "C"
