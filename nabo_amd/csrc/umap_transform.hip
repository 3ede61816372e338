// UMAP transform: target cells placed in a fitted reference embedding that does not move
// (include/nabo_umap_transform.h is the contract).
//
// Graph build, once per batch.  A group of W lanes (W the power of two >= k, at least 8) holds one target's list in
// registers, one entry per lane: the 64-step search for sigma and the row's mean, every sum a butterfly over the group
// (the header's TREE), then the memberships, their sum and the start.  The start is a sum in list order, so the lanes'
// products are handed round the group one position at a time and every lane adds them in that order.
//
// Optimise, the hot path.  The reference never moves, so a target needs nothing another target writes: UT_GROUP lanes
// share a target and keep, for the whole run, its position, their arcs' reference positions and the arcs' schedule in
// registers.  All epochs of a run are one launch with no synchronisation; the only memory traffic of an epoch is the
// gathers of the negative samples, UT_BATCH of them in flight per lane: their indices are hashed and their positions
// requested before the first is used.  A lane whose arc does not fire in an epoch idles through it.  Each lane sums in
// its own fixed order, the lanes are added by a butterfly, and every lane of the group moves its copy of the position by
// the same bits.  At the end the position and the schedule go back to memory, so that a later run continues.  No
// atomics, no LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "../../include/nabo_umap_transform.h"
#include "host_common.h"
#include "umap_common.h"

namespace nabo {

constexpr int UT_THREADS = 256;
constexpr int UT_GROUP = 16;    // lanes per target of the optimise kernel: part of the definition (the order of a target's sum)
constexpr int UT_BATCH = 4;     // negative samples whose gathers are in flight together
constexpr int UT_MAX_ARCS = (NABO_MAX_K + UT_GROUP - 1) / UT_GROUP;   // arcs a lane may hold

// B', C' and the start of one target per W lanes.  dist NULL: memb is given and sigma reads 0.
template <int W, int DIMS>
__global__ __launch_bounds__(UT_THREADS) void umap_transform_graph_kernel(const int64_t *__restrict__ idx, const double *__restrict__ dist,
                                                                          int64_t m, int k, double target, const double *__restrict__ Y,
                                                                          double *__restrict__ sigma, double *__restrict__ memb,
                                                                          double *__restrict__ y0, double *__restrict__ y)
{
    const int64_t i = ((int64_t)blockIdx.x * UT_THREADS + threadIdx.x) / W;
    const int t = threadIdx.x % W;
    const bool live = i < m, have = live && t < k;
    double a = 0.0, sg = 0.0;
    if (dist) {
        const double d = have ? dist[i * k + t] : 0.0;
        const bool term = have && t >= 1;
        double lo = 0.0, hi = std::numeric_limits<double>::infinity(), mid = 1.0;
        bool done = !live;
        for (int step = 0; step < 64; ++step) {
            double v = 0.0;
            if (term) v = d > 0.0 ? exp(-(d / mid)) : 1.0;
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
        const double mean = umap_tree<W>(d) / (double)k;
        sg = fmax(mid, 1e-3 * mean);
        if (have) a = (d <= 0.0 || sg == 0.0) ? 1.0 : exp(-(d / sg));
    } else if (have)
        a = memb[i * k + t];
    const double s = umap_tree<W>(a);
    const double wgt = a / s;
    const int64_t j = have ? idx[i * k + t] : 0;
    double prod[DIMS], acc[DIMS];
#pragma unroll
    for (int c = 0; c < DIMS; ++c) {
        prod[c] = have ? wgt * Y[j * DIMS + c] : 0.0;
        acc[c] = 0.0;
    }
    for (int u = 0; u < k; ++u)
#pragma unroll
        for (int c = 0; c < DIMS; ++c) acc[c] += __shfl(prod[c], u, W);
    if (have && dist) memb[i * k + t] = a;
    if (live && t == 0) {
        sigma[i] = sg;
#pragma unroll
        for (int c = 0; c < DIMS; ++c) y0[i * DIMS + c] = y[i * DIMS + c] = acc[c];
    }
}

// the first state of the schedule; an arc that is not live never fires (next = +inf)
__global__ __launch_bounds__(UT_THREADS) void umap_transform_schedule_kernel(int64_t mk, const double *__restrict__ memb, double n_epochs,
                                                                             double nsr, double *__restrict__ next, double *__restrict__ nneg)
{
    const int64_t q = (int64_t)blockIdx.x * UT_THREADS + threadIdx.x;
    if (q >= mk) return;
    const double a = memb[q], eps = 1.0 / a;
    next[q] = a >= 1.0 / n_epochs ? eps : std::numeric_limits<double>::infinity();
    nneg[q] = eps / nsr;
}

// A: list positions per lane (k <= A * UT_GROUP)
template <int DIMS, int A>
__global__ __launch_bounds__(UT_THREADS) void umap_transform_run_kernel(int64_t m, int k, const int64_t *__restrict__ idx,
                                                                        const double *__restrict__ memb, double *__restrict__ next,
                                                                        double *__restrict__ nneg, const double *__restrict__ Y,
                                                                        double *__restrict__ y, UmapTransformRun P,
                                                                        int64_t *__restrict__ n_attr, int64_t *__restrict__ n_neg,
                                                                        uint64_t *__restrict__ idx_sum)
{
    const int64_t i = ((int64_t)blockIdx.x * UT_THREADS + threadIdx.x) / UT_GROUP;
    const int l = threadIdx.x % UT_GROUP;
    const bool row = i < m;
    double yi[DIMS], yj[A][DIMS], eps[A], epn[A], nx[A], ng[A];
    uint64_t eh[A];             // G * (e + 1) of the arc's number e = (first_row + i) k + t_pos
    bool have[A];
#pragma unroll
    for (int r = 0; r < A; ++r) {
        const int t = l + r * UT_GROUP;
        have[r] = row && t < k;
        nx[r] = std::numeric_limits<double>::infinity();
        eps[r] = epn[r] = ng[r] = 0.0;
        eh[r] = 0;
#pragma unroll
        for (int c = 0; c < DIMS; ++c) yj[r][c] = 0.0;
        if (have[r]) {
            const int64_t q = i * k + t, j = idx[q];
            const double a = memb[q];
            eps[r] = 1.0 / a;
            epn[r] = eps[r] / P.nsr;
            nx[r] = next[q];
            ng[r] = nneg[q];
#pragma unroll
            for (int c = 0; c < DIMS; ++c) yj[r][c] = Y[j * DIMS + c];
            eh[r] = UM_GOLD * ((uint64_t)((P.first_row + i) * k + t) + 1);
        }
    }
#pragma unroll
    for (int c = 0; c < DIMS; ++c) yi[c] = row ? y[i * DIMS + c] : 0.0;
    int64_t na = 0, nn = 0;
    uint64_t ks = 0;
    for (int64_t t = P.t0; t < P.t1; ++t) {
        const double tf = (double)t, alpha = 0.25 * (1.0 - tf / P.n_epochs);
        const uint64_t s_t = umap_mix(P.seed + UM_GOLD * ((uint64_t)t + 1));
        double acc[DIMS];
#pragma unroll
        for (int c = 0; c < DIMS; ++c) acc[c] = 0.0;
#pragma unroll
        for (int r = 0; r < A; ++r) {
            if (!(nx[r] <= tf)) continue;
            {   // (i) attraction: everything is in registers
                double D[DIMS], d2 = 0.0;
#pragma unroll
                for (int c = 0; c < DIMS; ++c) {
                    D[c] = yi[c] - yj[r][c];
                    d2 += D[c] * D[c];
                }
                const double cf = d2 > 0.0 ? (P.ca * pow(d2, P.b - 1.0)) / (P.a * pow(d2, P.b) + 1.0) : 0.0;
#pragma unroll
                for (int c = 0; c < DIMS; ++c) acc[c] += umap_clip(cf * D[c]);
                ++na;
            }
            nx[r] += eps[r];
            // (ii) negative samples, UT_BATCH gathers in flight
            const int64_t ms = (int64_t)((tf - ng[r]) / epn[r]);
            const uint64_t se = umap_mix(s_t + eh[r]);
            for (int64_t p0 = 0; p0 < ms; p0 += UT_BATCH) {
                int64_t kk[UT_BATCH];
                double yk[UT_BATCH][DIMS];
#pragma unroll
                for (int q = 0; q < UT_BATCH; ++q) {
                    const uint64_t z = umap_mix(se + UM_GOLD * ((uint64_t)(p0 + q) + 1));
                    kk[q] = (int64_t)(((z >> 32) * (uint64_t)P.n_ref) >> 32);   // < n_ref whatever z is
#pragma unroll
                    for (int c = 0; c < DIMS; ++c) yk[q][c] = Y[kk[q] * DIMS + c];
                }
#pragma unroll
                for (int q = 0; q < UT_BATCH; ++q) {
                    if (!(p0 + q < ms)) continue;
                    ++nn;
                    ks += (uint64_t)kk[q];
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
            ng[r] += (double)ms * epn[r];
        }
        // (iii) every lane of the group holds the same sum and moves its copy of the position
#pragma unroll
        for (int c = 0; c < DIMS; ++c) yi[c] += alpha * umap_tree<UT_GROUP>(acc[c]);
    }
#pragma unroll
    for (int s = 1; s < UT_GROUP; s <<= 1) {
        na += (int64_t)__shfl_xor((long long)na, s, UT_GROUP);
        nn += (int64_t)__shfl_xor((long long)nn, s, UT_GROUP);
        ks += (uint64_t)__shfl_xor((unsigned long long)ks, s, UT_GROUP);
    }
#pragma unroll
    for (int r = 0; r < A; ++r)
        if (have[r]) {
            const int64_t q = i * k + l + r * UT_GROUP;
            next[q] = nx[r];
            nneg[q] = ng[r];
        }
    if (row && l == 0) {
#pragma unroll
        for (int c = 0; c < DIMS; ++c) y[i * DIMS + c] = yi[c];
        n_attr[i] = na;
        n_neg[i] = nn;
        idx_sum[i] = ks;
    }
}

int umap_transform_group() { return UT_GROUP; }

static int umap_transform_width(int k) { return k <= 8 ? 8 : k <= 16 ? 16 : k <= 32 ? 32 : 64; }

hipError_t umap_transform_graph_launch(int dims, int64_t m, int k, const int64_t *idx, const double *dist, const double *Y, double *sigma,
                                       double *memb, double *y0, double *y, hipStream_t st)
{
    const int W = umap_transform_width(k);
    const unsigned grid = (unsigned)((m * W + UT_THREADS - 1) / UT_THREADS);
    const double target = std::log2((double)k);
#define UT_GRAPH(WW, DD)                                                                                                           \
    hipLaunchKernelGGL((umap_transform_graph_kernel<WW, DD>), dim3(grid), dim3(UT_THREADS), 0, st, idx, dist, m, k, target, Y, sigma, \
                       memb, y0, y)
#define UT_GRAPH_W(WW)                                                                                                             \
    do {                                                                                                                           \
        if (dims == 2) UT_GRAPH(WW, 2);                                                                                            \
        else UT_GRAPH(WW, 3);                                                                                                      \
    } while (0)
    if (W == 8) UT_GRAPH_W(8);
    else if (W == 16) UT_GRAPH_W(16);
    else if (W == 32) UT_GRAPH_W(32);
    else UT_GRAPH_W(64);
#undef UT_GRAPH_W
#undef UT_GRAPH
    return hipGetLastError();
}

hipError_t umap_transform_schedule_launch(int64_t mk, const double *memb, double n_epochs, double nsr, double *next, double *nneg,
                                          hipStream_t st)
{
    hipLaunchKernelGGL(umap_transform_schedule_kernel, dim3((unsigned)((mk + UT_THREADS - 1) / UT_THREADS)), dim3(UT_THREADS), 0, st, mk,
                       memb, n_epochs, nsr, next, nneg);
    return hipGetLastError();
}

hipError_t umap_transform_run_launch(int dims, int64_t m, int k, const int64_t *idx, const double *memb, double *next, double *nneg,
                                     const double *Y, double *y, const UmapTransformRun &P, int64_t *n_attr, int64_t *n_neg,
                                     uint64_t *idx_sum, hipStream_t st)
{
    const unsigned grid = (unsigned)((m * UT_GROUP + UT_THREADS - 1) / UT_THREADS);
    const int arcs = (k + UT_GROUP - 1) / UT_GROUP;
    if (arcs < 1 || arcs > UT_MAX_ARCS) return hipErrorInvalidValue;
#define UT_RUN(DD, AA)                                                                                                            \
    hipLaunchKernelGGL((umap_transform_run_kernel<DD, AA>), dim3(grid), dim3(UT_THREADS), 0, st, m, k, idx, memb, next, nneg, Y, y, P, \
                       n_attr, n_neg, idx_sum)
#define UT_RUN_A(AA)                                                                                                              \
    do {                                                                                                                          \
        if (dims == 2) UT_RUN(2, AA);                                                                                             \
        else UT_RUN(3, AA);                                                                                                       \
    } while (0)
    if (arcs == 1) UT_RUN_A(1);
    else if (arcs == 2) UT_RUN_A(2);
    else if (arcs == 3) UT_RUN_A(3);
    else UT_RUN_A(4);
#undef UT_RUN_A
#undef UT_RUN
    return hipGetLastError();
}

}  // namespace nabo

using nabo::DevBuf;

static_assert(nabo::UT_MAX_ARCS == 4, "umap_transform_run_launch instantiates 1 .. 4 arcs per lane");

struct nabo_umap_transform {
    int device = 0, dims = 2, k = 0, g = 0;
    int64_t n_ref = 0, m = 0, first_row = 0, n_epochs = 100, epoch = 0;
    int nsr = 5;
    double gamma = 1.0, a = 1.577, b = 0.895;
    uint64_t seed = 0;
    bool have_batch = false, ran = false;
    nabo_index *ix = nullptr;   // the resident index of set_cells, over X
    DevBuf Y, X, Z, idx, dist, sigma, memb, y0, y, next, nneg, n_attr, n_neg, idx_sum;
    nabo::Events<2> ev;
    double ms[3] = {0, 0, 0};
};

namespace {

#define UT_RESERVE(buf, bytes)                  \
    do {                                        \
        const int rc__ = (buf).reserve(bytes);  \
        if (rc__) return rc__;                  \
    } while (0)

int ut_check_batch(const nabo_umap_transform *T, int64_t m, int64_t first_row, int32_t k)
{
    if (k < 2 || k > NABO_MAX_K) return nabo::api_fail(NABO_E_INVALID, "k=%d must be in [2, %d]", (int)k, NABO_MAX_K);
    if (k > T->n_ref) return nabo::api_fail(NABO_E_INVALID, "k=%d must not exceed n_ref=%lld", (int)k, (long long)T->n_ref);
    if (m < 1) return nabo::api_fail(NABO_E_INVALID, "m=%lld must be at least 1", (long long)m);
    if (m >= ((int64_t)1 << 31)) return nabo::api_fail(NABO_E_UNSUPPORTED, "m=%lld: a batch takes fewer than 2^31 rows", (long long)m);
    if (first_row < 0 || first_row > (std::numeric_limits<int64_t>::max() / k) - m - 1)
        return nabo::api_fail(NABO_E_INVALID, "first_row=%lld must not be negative and (first_row + m) * k must stay below 2^63", (long long)first_row);
    return NABO_OK;
}

int ut_check_idx(const nabo_umap_transform *T, int64_t m, int32_t k, const int64_t *idx)
{
    for (int64_t q = 0; q < m * k; ++q)
        if (idx[q] < 0 || idx[q] >= T->n_ref)
            return nabo::api_fail(NABO_E_INVALID, "idx[%lld][%d] = %lld is not a reference cell in [0, %lld)", (long long)(q / k), (int)(q % k),
                                  (long long)idx[q], (long long)T->n_ref);
    return NABO_OK;
}

// room for a batch's lists (the results' room is made by ut_build)
int ut_reserve_lists(nabo_umap_transform *T, int64_t m, int32_t k, bool with_dist)
{
    T->have_batch = false;
    UT_RESERVE(T->idx, (size_t)m * k * 8);
    if (with_dist) UT_RESERVE(T->dist, (size_t)m * k * 8);
    return NABO_OK;
}

int ut_schedule(nabo_umap_transform *T)
{
    HIP_TRY(nabo::umap_transform_schedule_launch(T->m * T->k, T->memb.as<double>(), (double)T->n_epochs, (double)T->nsr, T->next.as<double>(),
                                                 T->nneg.as<double>(), nullptr));
    T->epoch = 0;
    return NABO_OK;
}

// B', C' (from T->dist when from_dist, else T->memb is given) and the start of the batch whose lists are in T->idx
int ut_build(nabo_umap_transform *T, int64_t m, int64_t first_row, int32_t k, bool from_dist)
{
    T->have_batch = false;
    T->ran = false;
    T->m = m;
    T->first_row = first_row;
    T->k = k;
    const size_t mk = (size_t)m * k * 8, md = (size_t)m * T->dims * 8;
    UT_RESERVE(T->sigma, (size_t)m * 8);
    if (from_dist) UT_RESERVE(T->memb, mk);
    UT_RESERVE(T->y0, md);
    UT_RESERVE(T->y, md);
    UT_RESERVE(T->next, mk);
    UT_RESERVE(T->nneg, mk);
    UT_RESERVE(T->n_attr, (size_t)m * 8);
    UT_RESERVE(T->n_neg, (size_t)m * 8);
    UT_RESERVE(T->idx_sum, (size_t)m * 8);
    HIP_TRY(hipEventRecord(T->ev.ev[0], nullptr));
    HIP_TRY(nabo::umap_transform_graph_launch(T->dims, m, k, T->idx.as<int64_t>(), from_dist ? T->dist.as<double>() : nullptr,
                                              T->Y.as<double>(), T->sigma.as<double>(), T->memb.as<double>(), T->y0.as<double>(),
                                              T->y.as<double>(), nullptr));
    int rc = ut_schedule(T);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(T->ev.ev[1], nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    T->ms[0] = 0;
    HIP_TRY(T->ev.elapsed(0, 1, &T->ms[0]));
    T->have_batch = true;
    return NABO_OK;
}

int ut_need_batch(const nabo_umap_transform *T)
{
    if (!T) return nabo::api_fail(NABO_E_INVALID, "transform is NULL");
    if (!T->have_batch)
        return nabo::api_fail(NABO_E_INVALID, "no batch: call nabo_umap_transform_query, nabo_umap_transform_set_knn or nabo_umap_transform_set_graph first");
    return NABO_OK;
}

}  // namespace

extern "C" {

int nabo_umap_transform_geometry(int32_t *group)
{
    if (group) *group = nabo::UT_GROUP;
    return NABO_OK;
}

int nabo_umap_transform_create(nabo_umap_transform **out, int32_t device, int64_t n_ref, int32_t dims)
{
    if (!out) return nabo::api_fail(NABO_E_INVALID, "out is NULL");
    *out = nullptr;
    if (n_ref < 2) return nabo::api_fail(NABO_E_INVALID, "n_ref=%lld must be at least 2", (long long)n_ref);
    if (n_ref >= ((int64_t)1 << 31))
        return nabo::api_fail(NABO_E_UNSUPPORTED, "n_ref=%lld: the transform takes fewer than 2^31 reference cells", (long long)n_ref);
    if (dims != 2 && dims != 3) return nabo::api_fail(NABO_E_INVALID, "dims=%d must be 2 or 3", (int)dims);
    int rc = nabo::use_device(device);
    if (rc) return rc;
    return nabo::create_handle(out, device, "nabo_umap_transform_create", [&](nabo_umap_transform *T) -> int {
        T->n_ref = n_ref;
        T->dims = dims;
        const size_t yb = (size_t)n_ref * dims * 8;
        HIP_TRY(T->Y.alloc(yb));
        HIP_TRY(hipMemset(T->Y.p, 0, yb));
        HIP_TRY(T->ev.create());
        return NABO_OK;
    });
}

void nabo_umap_transform_destroy(nabo_umap_transform *T)
{
    if (!T) return;
    (void)hipSetDevice(T->device);
    if (T->ix) (void)nabo_index_destroy(T->ix);
    delete T;
}

int nabo_umap_transform_set_params(nabo_umap_transform *T, int64_t n_epochs, int32_t negative_sample_rate, double repulsion_strength,
                                   double a, double b, uint64_t seed)
{
    if (!T) return nabo::api_fail(NABO_E_INVALID, "transform is NULL");
    if (n_epochs < 1) return nabo::api_fail(NABO_E_INVALID, "n_epochs=%lld must be at least 1", (long long)n_epochs);
    if (negative_sample_rate < 1) return nabo::api_fail(NABO_E_INVALID, "negative_sample_rate=%d must be at least 1", (int)negative_sample_rate);
    if (!std::isfinite(repulsion_strength) || !std::isfinite(a) || !std::isfinite(b) || !(a > 0.0) || !(b > 0.0))
        return nabo::api_fail(NABO_E_INVALID, "repulsion_strength, a and b must be finite, a and b positive");
    T->n_epochs = n_epochs;
    T->nsr = negative_sample_rate;
    T->gamma = repulsion_strength;
    T->a = a;
    T->b = b;
    T->seed = seed;
    T->epoch = 0;
    if (!T->have_batch) return NABO_OK;
    int rc = nabo::use_device(T->device);
    if (rc) return rc;
    if ((rc = ut_schedule(T))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return NABO_OK;
}

int nabo_umap_transform_set_embedding(nabo_umap_transform *T, const double *Y)
{
    if (!T || !Y) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    const size_t cnt = (size_t)T->n_ref * T->dims;
    for (size_t q = 0; q < cnt; ++q)
        if (!std::isfinite(Y[q])) return nabo::api_fail(NABO_E_INVALID, "Y[%zu][%zu] is not finite", q / T->dims, q % T->dims);
    int rc = nabo::use_device(T->device);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(T->Y.p, Y, cnt * 8, hipMemcpyHostToDevice));
    return NABO_OK;
}

int nabo_umap_transform_set_cells(nabo_umap_transform *T, const double *X, int32_t g, int32_t metric, double dist_factor)
{
    if (!T || !X) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    if (g < 1) return nabo::api_fail(NABO_E_INVALID, "g=%d must be at least 1", (int)g);
    int rc = nabo::use_device(T->device);
    if (rc) return rc;
    if (T->ix) (void)nabo_index_destroy(T->ix);
    T->ix = nullptr;
    T->g = 0;
    nabo_index *ix = nullptr;
    if ((rc = nabo_index_create(&ix, T->device, T->n_ref, g, metric, dist_factor, 0))) return rc;
    auto fill = [&]() -> int {
        HIP_TRY(T->X.alloc((size_t)T->n_ref * g * 8));
        HIP_TRY(hipMemcpy(T->X.p, X, (size_t)T->n_ref * g * 8, hipMemcpyHostToDevice));
        return nabo_index_set_ref(ix, T->X.as<double>(), 1, nullptr);
    };
    if ((rc = fill())) {
        (void)nabo_index_destroy(ix);
        return rc;
    }
    T->ix = ix;
    T->g = g;
    return NABO_OK;
}

int nabo_umap_transform_query(nabo_umap_transform *T, int64_t m, int64_t first_row, const double *Z, int32_t k)
{
    if (!T || !Z) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    if (!T->ix) return nabo::api_fail(NABO_E_INVALID, "no reference cells: call nabo_umap_transform_set_cells first");
    int rc = ut_check_batch(T, m, first_row, k);
    if (rc) return rc;
    if ((rc = nabo::use_device(T->device))) return rc;
    if ((rc = ut_reserve_lists(T, m, k, true))) return rc;
    UT_RESERVE(T->Z, (size_t)m * T->g * 8);
    HIP_TRY(hipMemcpy(T->Z.p, Z, (size_t)m * T->g * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipEventRecord(T->ev.ev[0], nullptr));
    if ((rc = nabo_index_query(T->ix, T->Z.as<double>(), 1, m, k, 0, T->idx.as<int64_t>(), T->dist.as<double>(), 1))) return rc;
    HIP_TRY(hipEventRecord(T->ev.ev[1], nullptr));
    HIP_TRY(hipDeviceSynchronize());
    T->ms[1] = 0;
    HIP_TRY(T->ev.elapsed(0, 1, &T->ms[1]));
    return ut_build(T, m, first_row, k, true);
}

int nabo_umap_transform_set_knn(nabo_umap_transform *T, int64_t m, int64_t first_row, const int64_t *idx, const double *dist, int32_t k)
{
    if (!T || !idx || !dist) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    int rc = ut_check_batch(T, m, first_row, k);
    if (rc) return rc;
    if ((rc = ut_check_idx(T, m, k, idx))) return rc;
    for (int64_t i = 0; i < m; ++i)
        for (int t = 0; t < k; ++t) {
            const int64_t q = i * k + t;
            if (!std::isfinite(dist[q]) || dist[q] < 0.0 || (t > 0 && dist[q] < dist[q - 1]))
                return nabo::api_fail(NABO_E_INVALID, "dist[%lld][%d] is not finite, is negative or is below its predecessor", (long long)i, t);
        }
    if ((rc = nabo::use_device(T->device))) return rc;
    if ((rc = ut_reserve_lists(T, m, k, true))) return rc;
    const size_t nb = (size_t)m * k * 8;
    HIP_TRY(hipMemcpy(T->idx.p, idx, nb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(T->dist.p, dist, nb, hipMemcpyHostToDevice));
    T->ms[1] = 0;
    return ut_build(T, m, first_row, k, true);
}

int nabo_umap_transform_set_graph(nabo_umap_transform *T, int64_t m, int64_t first_row, const int64_t *idx, const double *memb, int32_t k)
{
    if (!T || !idx || !memb) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    int rc = ut_check_batch(T, m, first_row, k);
    if (rc) return rc;
    if ((rc = ut_check_idx(T, m, k, idx))) return rc;
    for (int64_t q = 0; q < m * k; ++q)
        if (!std::isfinite(memb[q]) || memb[q] < 0.0 || memb[q] > 1.0)
            return nabo::api_fail(NABO_E_INVALID, "memb[%lld][%d] is not a finite value in [0, 1]", (long long)(q / k), (int)(q % k));
    if ((rc = nabo::use_device(T->device))) return rc;
    if ((rc = ut_reserve_lists(T, m, k, false))) return rc;
    const size_t nb = (size_t)m * k * 8;
    UT_RESERVE(T->memb, nb);
    HIP_TRY(hipMemcpy(T->idx.p, idx, nb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(T->memb.p, memb, nb, hipMemcpyHostToDevice));
    T->ms[1] = 0;
    return ut_build(T, m, first_row, k, false);
}

int nabo_umap_transform_get_graph(nabo_umap_transform *T, double *sigma, double *memb, double *y0)
{
    int rc = ut_need_batch(T);
    if (rc) return rc;
    if ((rc = nabo::use_device(T->device))) return rc;
    if (sigma) HIP_TRY(hipMemcpy(sigma, T->sigma.p, (size_t)T->m * 8, hipMemcpyDeviceToHost));
    if (memb) HIP_TRY(hipMemcpy(memb, T->memb.p, (size_t)T->m * T->k * 8, hipMemcpyDeviceToHost));
    if (y0) HIP_TRY(hipMemcpy(y0, T->y0.p, (size_t)T->m * T->dims * 8, hipMemcpyDeviceToHost));
    return NABO_OK;
}

int nabo_umap_transform_set_positions(nabo_umap_transform *T, const double *y)
{
    int rc = ut_need_batch(T);
    if (rc) return rc;
    if (!y) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    const size_t cnt = (size_t)T->m * T->dims;
    for (size_t q = 0; q < cnt; ++q)
        if (!std::isfinite(y[q])) return nabo::api_fail(NABO_E_INVALID, "y[%zu][%zu] is not finite", q / T->dims, q % T->dims);
    if ((rc = nabo::use_device(T->device))) return rc;
    HIP_TRY(hipMemcpy(T->y.p, y, cnt * 8, hipMemcpyHostToDevice));
    return NABO_OK;
}

int nabo_umap_transform_get_positions(nabo_umap_transform *T, double *y)
{
    int rc = ut_need_batch(T);
    if (rc) return rc;
    if (!y) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    if ((rc = nabo::use_device(T->device))) return rc;
    HIP_TRY(hipMemcpy(y, T->y.p, (size_t)T->m * T->dims * 8, hipMemcpyDeviceToHost));
    return NABO_OK;
}

int nabo_umap_transform_rewind(nabo_umap_transform *T)
{
    int rc = ut_need_batch(T);
    if (rc) return rc;
    if ((rc = nabo::use_device(T->device))) return rc;
    if ((rc = ut_schedule(T))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return NABO_OK;
}

int nabo_umap_transform_run(nabo_umap_transform *T, int64_t n_run, int64_t *done)
{
    if (done) *done = 0;
    int rc = ut_need_batch(T);
    if (rc) return rc;
    if (n_run < 0) return nabo::api_fail(NABO_E_INVALID, "n_run=%lld is negative", (long long)n_run);
    if ((rc = nabo::use_device(T->device))) return rc;
    n_run = std::min<int64_t>(n_run, T->n_epochs - T->epoch);
    T->ms[2] = 0;
    if (n_run <= 0) return NABO_OK;
    nabo::UmapTransformRun P;
    P.a = T->a;
    P.b = T->b;
    P.ca = (-2.0 * T->a) * T->b;
    P.cr = (2.0 * T->gamma) * T->b;
    P.n_epochs = (double)T->n_epochs;
    P.nsr = (double)T->nsr;
    P.t0 = T->epoch;
    P.t1 = T->epoch + n_run;
    P.seed = T->seed;
    P.first_row = T->first_row;
    P.n_ref = T->n_ref;
    HIP_TRY(hipEventRecord(T->ev.ev[0], nullptr));
    HIP_TRY(nabo::umap_transform_run_launch(T->dims, T->m, T->k, T->idx.as<int64_t>(), T->memb.as<double>(), T->next.as<double>(),
                                            T->nneg.as<double>(), T->Y.as<double>(), T->y.as<double>(), P, T->n_attr.as<int64_t>(),
                                            T->n_neg.as<int64_t>(), T->idx_sum.as<uint64_t>(), nullptr));
    HIP_TRY(hipEventRecord(T->ev.ev[1], nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(T->ev.elapsed(0, 1, &T->ms[2]));
    T->epoch += n_run;
    T->ran = true;
    if (done) *done = n_run;
    return NABO_OK;
}

int nabo_umap_transform_last_run_counts(nabo_umap_transform *T, int64_t *n_attr, int64_t *n_neg, uint64_t *idx_sum)
{
    int rc = ut_need_batch(T);
    if (rc) return rc;
    if (!T->ran) return nabo::api_fail(NABO_E_INVALID, "no epoch has run on this batch");
    if ((rc = nabo::use_device(T->device))) return rc;
    const size_t nb = (size_t)T->m * 8;
    if (n_attr) HIP_TRY(hipMemcpy(n_attr, T->n_attr.p, nb, hipMemcpyDeviceToHost));
    if (n_neg) HIP_TRY(hipMemcpy(n_neg, T->n_neg.p, nb, hipMemcpyDeviceToHost));
    if (idx_sum) HIP_TRY(hipMemcpy(idx_sum, T->idx_sum.p, nb, hipMemcpyDeviceToHost));
    return NABO_OK;
}

int nabo_umap_transform_last_ms(nabo_umap_transform *T, double ms[3])
{
    if (!T || !ms) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    for (int i = 0; i < 3; ++i) ms[i] = T->ms[i];
    return NABO_OK;
}

}  // extern "C"
