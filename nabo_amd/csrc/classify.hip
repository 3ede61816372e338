// Classification of target nodes into the reference's clusters (nabo/_graph.py:722-792 classify_target): per target
// node, the weight its edges put into every cluster, the best cluster, and whether it holds more than weight_frac of
// the node's total weight.
//
// The float64 sums are the contract: the reference adds a node's edge weights one by one in networkx adjacency order,
// which is the row's order with a repeated neighbour merged into its first position (carrying its last weight).  So a
// row is walked sequentially by ONE lane and the parallelism is across rows.  The edges of 64 consecutive rows are one
// contiguous span of (nbr, w): the wavefront stages it into LDS with coalesced loads -- the cluster of every neighbour
// is gathered there too, one 4-byte read per edge from a table that sits in L2 -- and every lane then walks its own
// row from LDS.  A span longer than the stage is cut at row boundaries; a single row longer than the stage is staged
// into a device scratch instead and walked by its lane from there.  The walk reads a row O(len^2) times (merging
// repeats, then one sum per cluster), cheap at k = 11..50; rows beyond CLS_MAX_ROW edges are refused by the ABI.
//
// No per-cluster accumulators (n_clusters is a run-time number): a row's clusters are summed one after the other, each
// sum taking the cluster's edges in row order -- the same additions in the same order as one accumulator per cluster.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nabo {

constexpr int CLS_LANES = 64;       // rows per batch: one per lane of the workgroup's single wavefront
constexpr int CLS_CAP = 1024;       // edges staged at a time, 16 B each (16 KiB of LDS: ten workgroups per CU)
constexpr int CLS_MAX_ROW = 4096;   // longest row accepted: one lane walks a row with O(len^2) reads

// One row of `len` staged edges: nb neighbour, wt weight, cl the neighbour's cluster or -1.  Overwrites wt (merged
// weight at first positions) and cl (-2: repeated neighbour, -1: the edge counts for no cluster).
__device__ __forceinline__ void classify_row(const int32_t *nb, double *wt, int32_t *cl, int len, int32_t n_clusters,
                                             double weight_frac, int64_t min_degree, double min_weight, int32_t &label,
                                             double &best_out, double &total_out)
{
    int64_t deg = 0;
    double total = 0.0;
    for (int i = 0; i < len; ++i) {
        const int32_t v = nb[i];
        bool first = true;
        for (int j = 0; j < i; ++j)
            if (nb[j] == v) {
                first = false;
                break;
            }
        if (!first) {
            cl[i] = -2;
            continue;
        }
        double x = wt[i];
        for (int j = i + 1; j < len; ++j)
            if (nb[j] == v) x = wt[j];
        wt[i] = x;
        ++deg;
        total += x;
        if (!(x > min_weight) || cl[i] < 0) cl[i] = -1;
    }
    double best = 0.0;
    int32_t bestc = -1, present = 0;
    for (int i = 0; i < len; ++i) {
        const int32_t c = cl[i];
        if (c < 0) continue;
        bool seen = false;
        for (int j = 0; j < i; ++j)
            if (cl[j] == c) {
                seen = true;
                break;
            }
        if (seen) continue;
        double s = 0.0;
        for (int j = i; j < len; ++j)
            if (cl[j] == c) s += wt[j];
        ++present;
        if (bestc < 0 || s > best || (s == best && c < bestc)) {
            best = s;
            bestc = c;
        }
    }
    // a cluster without a counted edge holds 0: it is the best one only when no sum is positive
    if (present < n_clusters && (bestc < 0 || !(best > 0.0))) {
        int32_t a = 0;
        for (;; ++a) {
            bool here = false;
            for (int j = 0; j < len; ++j)
                if (cl[j] == a) {
                    here = true;
                    break;
                }
            if (!here) break;
        }
        if (bestc < 0 || best < 0.0 || (best == 0.0 && a < bestc)) {
            best = 0.0;
            bestc = a;
        }
    }
    const double need = weight_frac * total;
    label = (deg >= min_degree && best > need) ? bestc : -1;
    best_out = best;
    total_out = total;
}

__global__ __launch_bounds__(CLS_LANES) void classify_rows_kernel(
    const int32_t *__restrict__ ref_cluster, int32_t n_clusters, int64_t n_targets, const int64_t *__restrict__ ptr,
    const int64_t *__restrict__ nbr, const double *__restrict__ w, double weight_frac, int64_t min_degree, double min_weight,
    int32_t *__restrict__ long_nb, double *__restrict__ long_wt, int32_t *__restrict__ long_cl, int32_t *__restrict__ out_label,
    double *__restrict__ out_best, double *__restrict__ out_total)
{
    __shared__ double s_wt[CLS_CAP];
    __shared__ int32_t s_nb[CLS_CAP], s_cl[CLS_CAP];
    const int lane = threadIdx.x;
    const int64_t r = (int64_t)blockIdx.x * CLS_LANES + lane;
    const bool have = r < n_targets;
    const int64_t rr = have ? r : n_targets;
    const int64_t a = ptr[rr], b = have ? ptr[rr + 1] : a;      // lanes past the end hold an empty row at the very end
    int32_t label = -1;
    double best = 0.0, total = 0.0;
    int done = 0;                                               // rows of this batch answered so far (uniform)
    while (done < CLS_LANES) {
        const int64_t base = __shfl((long long)a, done, CLS_LANES);
        // rows done, done+1, ... that end within the stage: ptr is monotone, so they are a run from `done`
        const unsigned long long fits = __ballot(lane >= done && b - base <= CLS_CAP) >> done;
        const int run = ~fits ? __ffsll(~fits) - 1 : CLS_LANES - done;
        if (run == 0) {
            // one row longer than the stage: all lanes copy it into the scratch, its lane walks it there
            const int64_t len = __shfl((long long)b, done, CLS_LANES) - base;
            for (int64_t e = lane; e < len; e += CLS_LANES) {
                const int64_t v = nbr[base + e];
                long_nb[base + e] = (int32_t)v;
                long_wt[base + e] = w[base + e];
                long_cl[base + e] = ref_cluster[v];
            }
            __threadfence();
            __syncthreads();
            if (lane == done)
                classify_row(long_nb + base, long_wt + base, long_cl + base, (int)len, n_clusters, weight_frac, min_degree,
                             min_weight, label, best, total);
            done += 1;
            continue;
        }
        const int span = (int)(__shfl((long long)b, done + run - 1, CLS_LANES) - base);
        for (int e = lane; e < span; e += CLS_LANES) {
            const int64_t v = nbr[base + e];
            s_nb[e] = (int32_t)v;
            s_wt[e] = w[base + e];
            s_cl[e] = ref_cluster[v];
        }
        __syncthreads();
        if (lane >= done && lane < done + run) {
            const int off = (int)(a - base);
            classify_row(s_nb + off, s_wt + off, s_cl + off, (int)(b - a), n_clusters, weight_frac, min_degree, min_weight,
                         label, best, total);
        }
        __syncthreads();
        done += run;
    }
    if (have) {
        out_label[r] = label;
        if (out_best) out_best[r] = best;
        if (out_total) out_total[r] = total;
    }
}

// counts[c] = nodes labelled c, counts[n_clusters] = nodes labelled -1
constexpr int CLS_HIST = 1024;

__global__ __launch_bounds__(256) void classify_count_kernel(const int32_t *__restrict__ label, int64_t n, int32_t n_clusters,
                                                             unsigned long long *__restrict__ counts)
{
    __shared__ unsigned int h[CLS_HIST];
    const bool in_lds = n_clusters < CLS_HIST;
    if (in_lds)
        for (int i = threadIdx.x; i <= n_clusters; i += 256) h[i] = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int32_t l = label[i];
        const int32_t slot = l < 0 ? n_clusters : l;
        if (in_lds) atomicAdd(&h[slot], 1u);
        else atomicAdd(&counts[slot], 1ull);
    }
    __syncthreads();
    if (in_lds)
        for (int i = threadIdx.x; i <= n_clusters; i += 256)
            if (h[i]) atomicAdd(&counts[i], (unsigned long long)h[i]);
}

hipError_t classify_launch(const int32_t *ref_cluster, int32_t n_clusters, int64_t n_targets, const int64_t *ptr,
                           const int64_t *nbr, const double *w, double weight_frac, int64_t min_degree, double min_weight,
                           int32_t *long_nb, double *long_wt, int32_t *long_cl, int32_t *out_label, double *out_best,
                           double *out_total, int64_t *out_counts, hipStream_t st)
{
    if (n_targets > 0) {
        const unsigned grid = (unsigned)((n_targets + CLS_LANES - 1) / CLS_LANES);
        hipLaunchKernelGGL(classify_rows_kernel, dim3(grid), dim3(CLS_LANES), 0, st, ref_cluster, n_clusters, n_targets, ptr, nbr, w,
                           weight_frac, min_degree, min_weight, long_nb, long_wt, long_cl, out_label, out_best, out_total);
    }
    if (out_counts) {
        hipError_t e = hipMemsetAsync(out_counts, 0, ((size_t)n_clusters + 1) * 8, st);
        if (e != hipSuccess) return e;
        if (n_targets > 0) {
            const int64_t want = (n_targets + 256 * 16 - 1) / (256 * 16);
            hipLaunchKernelGGL(classify_count_kernel, dim3((unsigned)(want > 1024 ? 1024 : want)), dim3(256), 0, st,
                               (const int32_t *)out_label, n_targets, n_clusters, (unsigned long long *)out_counts);
        }
    }
    return hipGetLastError();
}

int classify_stage_edges() { return CLS_CAP; }
int classify_max_row() { return CLS_MAX_ROW; }

}  // namespace nabo

// ---- C ABI (include/nabo_cluster.h) -------------------------------------------------------------------------------
#include "../../include/nabo_cluster.h"
#include "host_common.h"

namespace {

using nabo::DevBuf;

// device time of the last calls on this thread: [0] nabo_classify_targets kernels, [1] nabo_refgraph_set_levels sweeps
thread_local double g_device_ms[2] = {0, 0};

}  // namespace

namespace nabo {
void cluster_set_device_ms(int which, double ms) { g_device_ms[which] = ms; }
}  // namespace nabo

extern "C" {

int nabo_classify_targets(int32_t device, int64_t n_ref, const int32_t *ref_cluster, int32_t n_clusters, int64_t n_targets,
                          const int64_t *ptr, const int64_t *nbr, const double *w, double weight_frac, int64_t min_degree,
                          double min_weight, int32_t *out_label, double *out_best, double *out_total, int64_t *out_counts)
{
    if (n_ref < 0 || n_ref >= ((int64_t)1 << 31) - 1) return nabo::api_fail(NABO_E_INVALID, "n_ref=%lld out of range [0, 2^31 - 1)", (long long)n_ref);
    if (n_clusters < 1) return nabo::api_fail(NABO_E_INVALID, "n_clusters=%d: at least one cluster is needed", (int)n_clusters);
    if (n_targets < 0 || n_targets >= ((int64_t)1 << 37)) return nabo::api_fail(NABO_E_INVALID, "n_targets=%lld out of range", (long long)n_targets);
    if (n_ref > 0 && !ref_cluster) return nabo::api_fail(NABO_E_INVALID, "ref_cluster is NULL");
    if (ptr && n_targets > 0 && !out_label) return nabo::api_fail(NABO_E_INVALID, "out_label is NULL");
    int rc = nabo::check_csr_ptr("ptr", "row", n_targets, ptr);
    if (rc) return rc;
    int64_t longest = 0;
    for (int64_t i = 0; i < n_targets; ++i) longest = ptr[i + 1] - ptr[i] > longest ? ptr[i + 1] - ptr[i] : longest;
    if (longest > nabo::classify_max_row())
        return nabo::api_fail(NABO_E_UNSUPPORTED, "a row of %lld edges: at most %d per target node", (long long)longest, nabo::classify_max_row());
    const int64_t E = ptr[n_targets];
    if (E > 0 && (!nbr || !w)) return nabo::api_fail(NABO_E_INVALID, "nbr or w is NULL");
    for (int64_t e = 0; e < E; ++e)
        if (nbr[e] < 0 || nbr[e] >= n_ref)
            return nabo::api_fail(NABO_E_INVALID, "nbr[%lld] = %lld is not a reference node in [0, %lld)", (long long)e, (long long)nbr[e], (long long)n_ref);
    for (int64_t i = 0; i < n_ref; ++i)
        if (ref_cluster[i] < -1 || ref_cluster[i] >= n_clusters)
            return nabo::api_fail(NABO_E_INVALID, "ref_cluster[%lld] = %d is not -1 or a cluster in [0, %d)", (long long)i, (int)ref_cluster[i], (int)n_clusters);
    if ((rc = nabo::use_device(device))) return rc;

    const bool scratch = longest > nabo::classify_stage_edges();
    DevBuf d_cl, d_ptr, d_nbr, d_w, d_lab, d_best, d_tot, d_cnt, l_nb, l_wt, l_cl;
    HIP_TRY(d_cl.alloc((size_t)n_ref * 4));
    HIP_TRY(d_ptr.alloc((size_t)(n_targets + 1) * 8));
    HIP_TRY(d_nbr.alloc((size_t)E * 8));
    HIP_TRY(d_w.alloc((size_t)E * 8));
    HIP_TRY(d_lab.alloc((size_t)n_targets * 4));
    if (out_best) HIP_TRY(d_best.alloc((size_t)n_targets * 8));
    if (out_total) HIP_TRY(d_tot.alloc((size_t)n_targets * 8));
    if (out_counts) HIP_TRY(d_cnt.alloc(((size_t)n_clusters + 1) * 8));
    if (scratch) {
        HIP_TRY(l_nb.alloc((size_t)E * 4));
        HIP_TRY(l_wt.alloc((size_t)E * 8));
        HIP_TRY(l_cl.alloc((size_t)E * 4));
    }
    hipStream_t st = nullptr;
    if (n_ref) HIP_TRY(hipMemcpyAsync(d_cl.p, ref_cluster, (size_t)n_ref * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_ptr.p, ptr, (size_t)(n_targets + 1) * 8, hipMemcpyHostToDevice, st));
    if (E) {
        HIP_TRY(hipMemcpyAsync(d_nbr.p, nbr, (size_t)E * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_w.p, w, (size_t)E * 8, hipMemcpyHostToDevice, st));
    }
    nabo::Events<2> events;
    HIP_TRY(events.create());
    HIP_TRY(hipEventRecord(events.ev[0], st));
    HIP_TRY(nabo::classify_launch(d_cl.as<int32_t>(), n_clusters, n_targets, d_ptr.as<int64_t>(), d_nbr.as<int64_t>(), d_w.as<double>(),
                                  weight_frac, min_degree, min_weight, l_nb.as<int32_t>(), l_wt.as<double>(), l_cl.as<int32_t>(),
                                  d_lab.as<int32_t>(), out_best ? d_best.as<double>() : nullptr, out_total ? d_tot.as<double>() : nullptr,
                                  out_counts ? d_cnt.as<int64_t>() : nullptr, st));
    HIP_TRY(hipEventRecord(events.ev[1], st));
    HIP_TRY(hipEventSynchronize(events.ev[1]));
    double ms = 0;
    HIP_TRY(events.elapsed(0, 1, &ms));
    g_device_ms[0] = ms;
    if (n_targets) {
        HIP_TRY(hipMemcpyAsync(out_label, d_lab.p, (size_t)n_targets * 4, hipMemcpyDeviceToHost, st));
        if (out_best) HIP_TRY(hipMemcpyAsync(out_best, d_best.p, (size_t)n_targets * 8, hipMemcpyDeviceToHost, st));
        if (out_total) HIP_TRY(hipMemcpyAsync(out_total, d_tot.p, (size_t)n_targets * 8, hipMemcpyDeviceToHost, st));
    }
    if (out_counts) HIP_TRY(hipMemcpyAsync(out_counts, d_cnt.p, ((size_t)n_clusters + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return NABO_OK;
}

int nabo_cluster_last_device_ms(double ms[2])
{
    if (!ms) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    ms[0] = g_device_ms[0];
    ms[1] = g_device_ms[1];
    return NABO_OK;
}

}  // extern "C"
