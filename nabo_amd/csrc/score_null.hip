// score_null.hip -- permutation null for mapping scores (gfx950).  EXTENSION: the reference has a mapping
// score (Graph.get_mapping_score, nabo/_graph.py:555-697: weighted degree of a target sample's edges on every
// reference node, x score_multiplier / n_target_nodes) but no permutation test; BASELINE.json's configs[4]
// asks for "1000-permutation null-model mapping scores".  Definition used here:
//
//   pooled target cells t = 0..n_t-1 with edges (t, r, w) onto reference nodes and a group flag (1 = the
//   sample of interest, n_A cells).   S_obs[r] = mult * sum_{e: r_e = r, group[t_e]} w_e / n_A.
//   Permutation p relabels the pooled cells: key(t,p) = top key_bits of splitmix64(seed, p, t),
//   T_p = the n_A-th smallest key, label_p[t] = (key <= T_p), n_p = #labelled (= n_A unless keys tie at T_p),
//   S_p[r] = mult * sum_{e: r_e = r, label_p[t_e]} w_e / n_p.
//   Outputs per reference node: S_obs, n_ge = #{p: S_p >= S_obs}, mean and population sd of S_p over p (two-pass:
//   sd = sqrt(sum_p (S_p - mean)^2 / P)).
//
// Integer results (thresholds, labels, n_p, n_ge) are bit-exact against the oracle; edge sums run in float64 in
// CSR order like the oracle's.  HBM-bound byte work: a label BIT-matrix [n_t][ceil(P/32)] is built once
// (n_t * P hashes), the reduction then reads one 4-byte word per (edge, 32 permutations).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <vector>

#include "host_common.h"

namespace nabo {

__device__ __forceinline__ uint64_t null_key(uint64_t seed, uint32_t p, uint64_t t, int key_bits)
{
    uint64_t z = seed + (uint64_t)(p + 1u) * 0x9E3779B97F4A7C15ull + t * 0xD1B54A32D192ED03ull;
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z >> (64 - key_bits);
}

// One radix-select pass: histogram of the next 8 key bits among the cells whose key starts with prefix[p].
// grid = (blocks over cells, P); hist [P][256] must be zeroed by the caller.
__global__ __launch_bounds__(256) void null_hist_kernel(int64_t n_t, uint64_t seed, int key_bits,
                                                        const uint64_t *__restrict__ prefix, int done_bits,
                                                        unsigned int *__restrict__ hist)
{
    __shared__ unsigned int h[256];
    const uint32_t p = blockIdx.y;
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t pre = prefix[p];
    const int shift = key_bits - done_bits - 8;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_t; t += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t k = null_key(seed, p, (uint64_t)t, key_bits);
        if (done_bits == 0 || (k >> (key_bits - done_bits)) == pre) atomicAdd(&h[(k >> shift) & 0xFFu], 1u);
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&hist[(size_t)p * 256 + threadIdx.x], h[threadIdx.x]);
}

// Label bits: word w of cell t holds permutations 32w .. 32w+31; slot P (the first bit after the
// permutations) carries the observed grouping.
__global__ __launch_bounds__(256) void null_label_kernel(int64_t n_t, int P, int W, uint64_t seed, int key_bits,
                                                         const uint64_t *__restrict__ thr,
                                                         const uint8_t *__restrict__ group,
                                                         uint32_t *__restrict__ bits)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_t * W) return;
    const int64_t t = e / W;
    const int w = (int)(e - t * W);
    uint32_t word = 0;
    for (int b = 0; b < 32; ++b) {
        const int p = w * 32 + b;
        bool on = false;
        if (p < P) on = null_key(seed, (uint32_t)p, (uint64_t)t, key_bits) <= thr[p];
        else if (p == P) on = group[t] != 0;
        if (on) word |= 1u << b;
    }
    bits[e] = word;
}

// One workgroup per reference node (CSR row): thread q accumulates permutations q, q+256, ... (and slot P,
// the observed grouping) over the row's edges in order, then the row's statistics are reduced: the mean first, then
// the squared deviations from it (the scores stay in registers between the two tree reductions).
template <int NACC>
__global__ __launch_bounds__(256) void null_score_kernel(const int64_t *__restrict__ row_ptr,
                                                         const int64_t *__restrict__ edge_t,
                                                         const double *__restrict__ edge_w, int P, int W,
                                                         const uint32_t *__restrict__ bits,
                                                         const int64_t *__restrict__ n_lab, int64_t n_a,
                                                         double mult, double *__restrict__ out_obs,
                                                         int64_t *__restrict__ out_nge, double *__restrict__ out_mean,
                                                         double *__restrict__ out_sd)
{
    __shared__ double s_red[256];
    __shared__ unsigned int s_ge;
    __shared__ double s_obs;
    const int64_t r = blockIdx.x;
    const int q = threadIdx.x;
    double acc[NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = 0.0;
    if (q == 0) s_ge = 0;
    for (int64_t e = row_ptr[r]; e < row_ptr[r + 1]; ++e) {
        const double w = edge_w[e];
        const uint32_t *bw = bits + edge_t[e] * W;
#pragma unroll
        for (int i = 0; i < NACC; ++i) {
            const int p = q + 256 * i;
            if (p <= P) acc[i] = __dadd_rn(acc[i], ((bw[p >> 5] >> (p & 31)) & 1u) ? w : 0.0);
        }
    }
    // observed score: slot P
    if (q == (P & 255)) s_obs = __ddiv_rn(__dmul_rn(mult, acc[P >> 8]), (double)n_a);
    __syncthreads();
    const double obs = s_obs;
    double sum = 0.0;
    unsigned int ge = 0;
#pragma unroll
    for (int i = 0; i < NACC; ++i) {
        const int p = q + 256 * i;
        if (p < P) {
            const double s = __ddiv_rn(__dmul_rn(mult, acc[i]), (double)n_lab[p]);
            acc[i] = s;                       // kept for the second pass
            sum += s;
            ge += (s >= obs) ? 1u : 0u;
        }
    }
    s_red[q] = sum;
    if (ge) atomicAdd(&s_ge, ge);
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (q < o) s_red[q] += s_red[q + o];
        __syncthreads();
    }
    // two-pass: squared deviations from the mean.  sum(s^2)/P - mean^2 cancels to nothing once the spread of the
    // permuted scores falls below ~1e-8 of their size (a node every pooled cell has an equal edge to)
    const double mean = s_red[0] / (double)P;
    __syncthreads();
    double dev = 0.0;
#pragma unroll
    for (int i = 0; i < NACC; ++i) {
        const int p = q + 256 * i;
        if (p < P) {
            const double d = acc[i] - mean;
            dev += d * d;
        }
    }
    s_red[q] = dev;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (q < o) s_red[q] += s_red[q + o];
        __syncthreads();
    }
    if (q == 0) {
        out_obs[r] = obs;
        out_nge[r] = (int64_t)s_ge;
        out_mean[r] = mean;
        out_sd[r] = sqrt(s_red[0] / (double)P);
    }
}

hipError_t null_hist_launch(int64_t n_t, int P, uint64_t seed, int key_bits, const uint64_t *prefix, int done_bits,
                            unsigned int *hist, hipStream_t st)
{
    int64_t bx = (n_t + 255) / 256;
    if (bx > 1024) bx = 1024;
    hipLaunchKernelGGL(null_hist_kernel, dim3((unsigned)bx, (unsigned)P), dim3(256), 0, st, n_t, seed, key_bits, prefix,
                       done_bits, hist);
    return hipGetLastError();
}

hipError_t null_label_launch(int64_t n_t, int P, int W, uint64_t seed, int key_bits, const uint64_t *thr,
                             const uint8_t *group, uint32_t *bits, hipStream_t st)
{
    const int64_t tot = n_t * W;
    hipLaunchKernelGGL(null_label_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, n_t, P, W, seed,
                       key_bits, thr, group, bits);
    return hipGetLastError();
}

hipError_t null_score_launch(int64_t n_ref, const int64_t *row_ptr, const int64_t *edge_t, const double *edge_w, int P,
                             int W, const uint32_t *bits, const int64_t *n_lab, int64_t n_a, double mult,
                             double *out_obs, int64_t *out_nge, double *out_mean, double *out_sd, hipStream_t st)
{
    const int nacc = (P + 1 + 255) / 256;
#define NABO_NS(N)                                                                                                 \
    hipLaunchKernelGGL((null_score_kernel<N>), dim3((unsigned)n_ref), dim3(256), 0, st, row_ptr, edge_t, edge_w, P, W, \
                       bits, n_lab, n_a, mult, out_obs, out_nge, out_mean, out_sd)
    if (nacc <= 1) NABO_NS(1);
    else if (nacc <= 2) NABO_NS(2);
    else if (nacc <= 4) NABO_NS(4);
    else if (nacc <= 8) NABO_NS(8);
    else if (nacc <= 17) NABO_NS(17);
    else return hipErrorInvalidValue;
#undef NABO_NS
    return hipGetLastError();
}

}  // namespace nabo

// ---- C ABI (include/nabo_knn.h: nabo_score_null, nabo_score_null_edges) ----------------------------------------------------
using nabo::api_fail;
using nabo::DevBuf;
using nabo::use_device;

namespace {

// row_ptr != NULL: edges in CSR by reference node (edge_r unused); row_ptr == NULL: COO, E = n_edges, the CSR is built
// on the device by a stable sort (csr_build.hip).
int score_null_impl(int32_t device, int64_t n_ref, const int64_t *row_ptr, int64_t n_edges, const int64_t *edge_r,
                    const int64_t *edge_t, const double *edge_w, int64_t n_t, const uint8_t *group, int32_t n_perm,
                    uint64_t seed, int32_t key_bits, double multiplier, double *out_obs, int64_t *out_nge,
                    double *out_mean, double *out_sd, int64_t *out_sizes)
{
    const bool coo = row_ptr == nullptr;
    if (!group || !out_obs || !out_nge || !out_mean || !out_sd) return api_fail(NABO_E_INVALID, "NULL argument");
    if (n_ref < 1 || n_t < 1) return api_fail(NABO_E_INVALID, "empty operand");
    if (n_perm < 1 || n_perm > 4096) return api_fail(NABO_E_UNSUPPORTED, "n_perm=%d: 1..4096 supported", n_perm);
    if (key_bits < 8 || key_bits > 64 || key_bits % 8) return api_fail(NABO_E_INVALID, "key_bits must be 8, 16, .., 64");
    if (n_ref >= 0x7FFFFFFFll) return api_fail(NABO_E_UNSUPPORTED, "n_ref too large for one launch");
    const int64_t E = coo ? n_edges : row_ptr[n_ref];
    if (coo) {
        if (E < 0) return api_fail(NABO_E_INVALID, "n_edges < 0");
        if (E >= 0xFFFFFFFFll) return api_fail(NABO_E_UNSUPPORTED, "n_edges=%lld: fewer than 2^32-1 supported", (long long)E);
        if (E > 0 && !edge_r) return api_fail(NABO_E_INVALID, "NULL edge arrays");
    } else {
        if (row_ptr[0] != 0 || E < 0) return api_fail(NABO_E_INVALID, "row_ptr must start at 0");
        for (int64_t r = 0; r < n_ref; ++r)
            if (row_ptr[r + 1] < row_ptr[r]) return api_fail(NABO_E_INVALID, "row_ptr must be non-decreasing");
        if (E > 0 && (!edge_t || !edge_w)) return api_fail(NABO_E_INVALID, "NULL edge arrays");
        for (int64_t e = 0; e < E; ++e)
            if (edge_t[e] < 0 || edge_t[e] >= n_t) return api_fail(NABO_E_INVALID, "edge_t[%lld] out of range", (long long)e);
    }
    if (E > 0 && (!edge_t || !edge_w)) return api_fail(NABO_E_INVALID, "NULL edge arrays");
    int64_t n_a = 0;
    for (int64_t t = 0; t < n_t; ++t) n_a += group[t] ? 1 : 0;
    if (n_a < 1) return api_fail(NABO_E_INVALID, "the group of interest is empty");
    int rc = use_device(device);
    if (rc) return rc;
    const int P = n_perm, W = (P + 1 + 31) / 32;
    hipStream_t st = nullptr;
    DevBuf d_rp, d_et, d_ew, d_grp, d_pre, d_hist, d_bits, d_nl, d_obs, d_nge, d_mean, d_sd;
    DevBuf c_r, c_t, c_w, c_ka, c_kb, c_pa, c_pb, c_tmp, c_flag;          // COO staging + sort scratch
    if ((rc = d_rp.reserve((size_t)(n_ref + 1) * 8)) || (rc = d_et.reserve((size_t)(E ? E : 1) * 8)) ||
        (rc = d_ew.reserve((size_t)(E ? E : 1) * 8)) || (rc = d_grp.reserve((size_t)n_t)) ||
        (rc = d_pre.reserve((size_t)P * 8)) || (rc = d_hist.reserve((size_t)P * 256 * 4)) ||
        (rc = d_bits.reserve((size_t)n_t * W * 4)) || (rc = d_nl.reserve((size_t)P * 8)) ||
        (rc = d_obs.reserve((size_t)n_ref * 8)) || (rc = d_nge.reserve((size_t)n_ref * 8)) ||
        (rc = d_mean.reserve((size_t)n_ref * 8)) || (rc = d_sd.reserve((size_t)n_ref * 8)))
        return rc;
    if (!coo) {
        HIP_TRY(hipMemcpyAsync(d_rp.p, row_ptr, (size_t)(n_ref + 1) * 8, hipMemcpyHostToDevice, st));
        if (E) {
            HIP_TRY(hipMemcpyAsync(d_et.p, edge_t, (size_t)E * 8, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(d_ew.p, edge_w, (size_t)E * 8, hipMemcpyHostToDevice, st));
        }
    } else {
        size_t tb = 0;
        HIP_TRY(nabo::csr_sort_temp_bytes(E, n_ref, &tb));
        const size_t e1 = (size_t)(E ? E : 1);
        if ((rc = c_r.reserve(e1 * 8)) || (rc = c_t.reserve(e1 * 8)) || (rc = c_w.reserve(e1 * 8)) ||
            (rc = c_ka.reserve(e1 * 4)) || (rc = c_kb.reserve(e1 * 4)) || (rc = c_pa.reserve(e1 * 4)) ||
            (rc = c_pb.reserve(e1 * 4)) || (rc = c_tmp.reserve(tb ? tb : 1)) || (rc = c_flag.reserve(sizeof(unsigned int))))
            return rc;
        if (E) {
            HIP_TRY(hipMemcpyAsync(c_r.p, edge_r, (size_t)E * 8, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(c_t.p, edge_t, (size_t)E * 8, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(c_w.p, edge_w, (size_t)E * 8, hipMemcpyHostToDevice, st));
        }
        HIP_TRY(nabo::csr_build_launch(c_r.as<int64_t>(), c_t.as<int64_t>(), c_w.as<double>(), E, n_ref, n_t,
                                       c_ka.as<uint32_t>(), c_pa.as<uint32_t>(), c_kb.as<uint32_t>(), c_pb.as<uint32_t>(),
                                       c_tmp.p, tb, d_rp.as<int64_t>(), d_et.as<int64_t>(), d_ew.as<double>(),
                                       c_flag.as<unsigned int>(), st));
        unsigned int bad = 0;
        HIP_TRY(hipMemcpyAsync(&bad, c_flag.p, sizeof(bad), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (bad) return api_fail(NABO_E_INVALID, "%s out of range", (bad & 1u) ? "edge_ref" : "edge_t");
        DevBuf *stage[] = {&c_r, &c_t, &c_w, &c_ka, &c_kb, &c_pa, &c_pb, &c_tmp};
        for (DevBuf *b : stage) b->release();
    }
    HIP_TRY(hipMemcpyAsync(d_grp.p, group, (size_t)n_t, hipMemcpyHostToDevice, st));
    // radix select of the n_A-th smallest key of every permutation, 8 bits per pass
    std::vector<uint64_t> prefix((size_t)P, 0), below((size_t)P, 0), rank((size_t)P, (uint64_t)n_a);
    std::vector<int64_t> sizes((size_t)P, 0);
    std::vector<unsigned int> hist((size_t)P * 256);
    for (int done = 0; done < key_bits; done += 8) {
        HIP_TRY(hipMemcpyAsync(d_pre.p, prefix.data(), (size_t)P * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(d_hist.p, 0, (size_t)P * 256 * 4, st));
        HIP_TRY(nabo::null_hist_launch(n_t, P, seed, key_bits, d_pre.as<uint64_t>(), done, d_hist.as<unsigned int>(), st));
        HIP_TRY(hipMemcpyAsync(hist.data(), d_hist.p, (size_t)P * 256 * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (int p = 0; p < P; ++p) {
            const unsigned int *h = &hist[(size_t)p * 256];
            uint64_t cum = 0;
            int b = 0;
            for (; b < 256; ++b) {
                if (cum + h[b] >= rank[p]) break;
                cum += h[b];
            }
            if (b == 256) return api_fail(NABO_E_HIP, "internal: radix select lost rank (permutation %d)", p);
            prefix[p] = (prefix[p] << 8) | (uint64_t)b;
            below[p] += cum;
            rank[p] -= cum;
            if (done + 8 >= key_bits) sizes[p] = (int64_t)(below[p] + h[b]);      // keys <= T_p (ties at T_p included)
        }
    }
    HIP_TRY(hipMemcpyAsync(d_pre.p, prefix.data(), (size_t)P * 8, hipMemcpyHostToDevice, st));        // thresholds T_p
    HIP_TRY(hipMemcpyAsync(d_nl.p, sizes.data(), (size_t)P * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(nabo::null_label_launch(n_t, P, W, seed, key_bits, d_pre.as<uint64_t>(), d_grp.as<uint8_t>(), d_bits.as<uint32_t>(), st));
    HIP_TRY(nabo::null_score_launch(n_ref, d_rp.as<int64_t>(), d_et.as<int64_t>(), d_ew.as<double>(), P, W,
                                    d_bits.as<uint32_t>(), d_nl.as<int64_t>(), n_a, multiplier, d_obs.as<double>(),
                                    d_nge.as<int64_t>(), d_mean.as<double>(), d_sd.as<double>(), st));
    HIP_TRY(hipMemcpyAsync(out_obs, d_obs.p, (size_t)n_ref * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out_nge, d_nge.p, (size_t)n_ref * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out_mean, d_mean.p, (size_t)n_ref * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out_sd, d_sd.p, (size_t)n_ref * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (out_sizes) memcpy(out_sizes, sizes.data(), (size_t)P * 8);
    return NABO_OK;
}

}  // namespace

extern "C" {

int nabo_score_null(int32_t device, int64_t n_ref, const int64_t *row_ptr, const int64_t *edge_t,
                    const double *edge_w, int64_t n_t, const uint8_t *group, int32_t n_perm, uint64_t seed,
                    int32_t key_bits, double multiplier, double *out_obs, int64_t *out_nge, double *out_mean,
                    double *out_sd, int64_t *out_sizes)
{
    if (!row_ptr) return api_fail(NABO_E_INVALID, "NULL argument");
    return score_null_impl(device, n_ref, row_ptr, 0, nullptr, edge_t, edge_w, n_t, group, n_perm, seed, key_bits,
                           multiplier, out_obs, out_nge, out_mean, out_sd, out_sizes);
}

int nabo_score_null_edges(int32_t device, int64_t n_ref, int64_t n_edges, const int64_t *edge_ref, const int64_t *edge_t,
                          const double *edge_w, int64_t n_t, const uint8_t *group, int32_t n_perm, uint64_t seed,
                          int32_t key_bits, double multiplier, double *out_obs, int64_t *out_nge, double *out_mean,
                          double *out_sd, int64_t *out_sizes)
{
    return score_null_impl(device, n_ref, nullptr, n_edges, edge_ref, edge_t, edge_w, n_t, group, n_perm, seed, key_bits,
                           multiplier, out_obs, out_nge, out_mean, out_sd, out_sizes);
}

}  // extern "C"
