// Mann-Whitney differential expression over sparse gene columns (nabo/_marker.py:12-114 run_de_test): per gene and per
// (test set, control set) pair, the expressed fraction, the log2 fold change, 2*U1, the tie term and z.
//
// A gene's value in most cells is 0, and a rank test of two samples that are mostly zeros is decided by how many zeros
// each holds and by the order of the few nonzeros.  So zeros are never materialised: a chunk of gene columns is EXPANDED
// into one 64-bit key per (nonzero, set the cell belongs to) -- (gene, set) in the high word, the bits of the float32
// value (non-negative, so they order as unsigned integers) in the low word -- the keys are SORTED by rocPRIM's radix
// sort over just the bits in use, and one wavefront per (gene, pair) RANKS two sorted runs against each other.  The
// zeros of a set are its size minus its run's length.  The reference keeps the min(n_test, n_ctrl) largest control
// values: the tail of the control run, then as many zeros as are still needed.  2*U1 and the tie term come from binary
// searches of one run in the other plus the two zero blocks, in int64 only, so they are exact and do not depend on how
// the hardware orders anything; the means are float64 sums of float32 values.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <stdint.h>

#include "launch.h"

namespace nabo {

constexpr int DE_WAVE = 64;

// memberships per nonzero: how many keys the entry emits
__global__ __launch_bounds__(256) void de_count_kernel(const int32_t *__restrict__ cell, int64_t nnz,
                                                       const int64_t *__restrict__ inv_ptr, uint32_t *__restrict__ cnt)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nnz) return;
    const int32_t c = cell[e];
    cnt[e] = (uint32_t)(inv_ptr[c + 1] - inv_ptr[c]);
}

// gptr: the chunk's column pointers relative to its first nonzero, [n_genes_chunk + 1]
__global__ __launch_bounds__(256) void de_emit_kernel(const int32_t *__restrict__ cell, const float *__restrict__ val, int64_t nnz,
                                                      const int64_t *__restrict__ gptr, int32_t n_genes_chunk,
                                                      const float *__restrict__ sf, const int64_t *__restrict__ inv_ptr,
                                                      const int32_t *__restrict__ inv_set, const uint32_t *__restrict__ off,
                                                      int64_t n_sets, uint64_t *__restrict__ keys)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nnz) return;
    int32_t lo = 0, hi = n_genes_chunk;          // the last gene with gptr[g] <= e
    while (hi - lo > 1) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (gptr[mid] <= e) lo = mid;
        else hi = mid;
    }
    const int32_t c = cell[e];
    float v = val[e] * sf[c];                    // one float32 product, as the reference's `a * self.sf`
    if (v == 0.0f) v = 0.0f;                     // -0 -> +0: a stored zero sorts in front of its run and is counted as a zero
    const uint64_t base = (uint64_t)lo * (uint64_t)n_sets;
    uint64_t *out = keys + off[e];
    const int64_t a = inv_ptr[c], b = inv_ptr[c + 1];
    for (int64_t j = a; j < b; ++j) out[j - a] = ((base + (uint64_t)inv_set[j]) << 32) | (uint64_t)__float_as_uint(v);
}

// seg[s] = first sorted position whose (gene, set) word is >= s, for s in [0, n_seg]
__global__ __launch_bounds__(256) void de_segptr_kernel(const uint64_t *__restrict__ keys, int64_t n, int64_t n_seg,
                                                        int64_t *__restrict__ seg)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    const int64_t prev = i == 0 ? -1 : (int64_t)(keys[i - 1] >> 32);
    const int64_t cur = i == n ? n_seg : (int64_t)(keys[i] >> 32);
    for (int64_t s = prev + 1; s <= cur; ++s) seg[s] = i;
}

__device__ __forceinline__ uint32_t de_val(const uint64_t *run, int64_t i) { return (uint32_t)run[i]; }

// first position of the run with value >= x (strict = false) or > x (strict = true)
__device__ __forceinline__ int64_t de_bound(const uint64_t *run, int64_t len, uint32_t x, bool strict)
{
    int64_t lo = 0, hi = len;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        const uint32_t y = de_val(run, mid);
        if (strict ? y <= x : y < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int64_t de_wave_sum(int64_t v)
{
    for (int o = DE_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor((long long)v, o, DE_WAVE);
    return v;
}

__device__ __forceinline__ double de_wave_sum(double v)
{
    for (int o = DE_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, DE_WAVE);
    return v;
}

// status codes of include/nabo_de.h
constexpr int32_t DE_SKIP_GENE = 0, DE_SKIP_PAIR = 1, DE_ASYMPTOTIC = 2, DE_EXACT = 3, DE_EMPTY = 4;

// One wavefront per (gene of the chunk, pair).  Outputs are indexed [gene_local * n_pairs + pair]; the host has zeroed
// them, so a status writes only what it defines.
__global__ __launch_bounds__(DE_WAVE) void de_rank_kernel(
    const uint64_t *__restrict__ keys, const int64_t *__restrict__ seg, int64_t n_sets, const int64_t *__restrict__ set_size,
    int64_t n_pairs, const int32_t *__restrict__ pair_test, const int32_t *__restrict__ pair_ctrl, double exp_frac_thresh,
    double log2_fc_thresh, int32_t *__restrict__ out_status, int64_t *__restrict__ out_nz, int64_t *__restrict__ out_n1,
    int64_t *__restrict__ out_n2, int64_t *__restrict__ out_u2, int64_t *__restrict__ out_tie, double *__restrict__ out_lfc,
    double *__restrict__ out_z, double *__restrict__ out_rbc)
{
    const int lane = threadIdx.x;
    const int64_t o = blockIdx.x;
    const int64_t gl = o / n_pairs, p = o - gl * n_pairs;
    const int32_t ts = pair_test[p], cs = pair_ctrl[p];
    const int64_t n1 = set_size[ts], ng = set_size[cs];
    const int64_t sa = seg[gl * n_sets + ts], sb = seg[gl * n_sets + cs];
    const uint64_t *A = keys + sa, *B = keys + sb;
    int64_t la = seg[gl * n_sets + ts + 1] - sa, lb = seg[gl * n_sets + cs + 1] - sb;
    // stored zeros sit in front of a run: they are zeros like the cells a column does not list
    const int64_t za = de_bound(A, la, 0u, true), zb = de_bound(B, lb, 0u, true);
    A += za, la -= za;
    B += zb, lb -= zb;
    const int64_t n2 = n1 < ng ? n1 : ng;
    if (lane == 0) {
        out_nz[o] = la;
        out_n1[o] = n1;
        out_n2[o] = n2;
    }
    if ((double)la / (double)n1 < exp_frac_thresh) {
        if (lane == 0) out_status[o] = DE_SKIP_GENE;
        return;
    }
    if (ng == 0) {
        if (lane == 0) {
            out_status[o] = DE_EMPTY;
            out_lfc[o] = __longlong_as_double(0x7ff8000000000000ll);
        }
        return;
    }
    // the n2 largest control values: the tail of the run, then zeros
    const int64_t kept = lb < n2 ? lb : n2;
    B += lb - kept, lb = kept;
    const int64_t z1 = n1 - la, zc = n2 - kept;
    double sum_a = 0.0, sum_b = 0.0;
    for (int64_t i = lane; i < la; i += DE_WAVE) sum_a += (double)__uint_as_float(de_val(A, i));
    for (int64_t i = lane; i < lb; i += DE_WAVE) sum_b += (double)__uint_as_float(de_val(B, i));
    const double mean_a = de_wave_sum(sum_a) / (double)n1, mean_b = de_wave_sum(sum_b) / (double)n2;
    const double lfc = mean_b == 0.0 ? __longlong_as_double(0x7ff0000000000000ll) : log2(mean_a) - log2(mean_b);
    if (lfc < log2_fc_thresh) {
        if (lane == 0) {
            out_status[o] = DE_SKIP_PAIR;
            out_lfc[o] = lfc;
        }
        return;
    }
    // 2*U1 = sum over test values x of 2 * #{control < x} + #{control == x}; tie = sum of t^3 - t over tie groups
    int64_t u2 = 0, tie = 0;
    for (int64_t i = lane; i < la; i += DE_WAVE) {
        const uint32_t x = de_val(A, i);
        const int64_t lo = de_bound(B, lb, x, false), hi = de_bound(B, lb, x, true);
        u2 += 2 * (zc + lo) + (hi - lo);
        if (i == 0 || de_val(A, i - 1) != x) {
            const int64_t t = (de_bound(A, la, x, true) - i) + (hi - lo);
            tie += t * t * t - t;
        }
    }
    for (int64_t j = lane; j < lb; j += DE_WAVE) {
        const uint32_t y = de_val(B, j);
        if (j == 0 || de_val(B, j - 1) != y) {
            const int64_t q = de_bound(A, la, y, false);
            if (q == la || de_val(A, q) != y) {                 // a value of the control sample alone
                const int64_t t = de_bound(B, lb, y, true) - j;
                tie += t * t * t - t;
            }
        }
    }
    if (lane == 0) {
        const int64_t t0 = z1 + zc;
        u2 += z1 * zc;
        tie += t0 * t0 * t0 - t0;
    }
    u2 = de_wave_sum(u2);
    tie = de_wave_sum(tie);
    if (lane != 0) return;
    // scipy's _get_mwu_z, operation by operation (the build does not contract a*b+c)
    const double n1n2 = (double)(n1 * n2);
    const double u1 = (double)u2 / 2.0, uu2 = n1n2 - u1;
    const double u = u1 > uu2 ? u1 : uu2;
    const double mu = n1n2 / 2.0;
    const int64_t n = n1 + n2;
    const double s = sqrt(n1n2 / 12.0 * ((double)(n + 1) - (double)tie / (double)(n * (n - 1))));
    double num = u - mu;
    num -= 0.5;
    out_status[o] = ((n1 <= 8 || n2 <= 8) && tie == 0) ? DE_EXACT : DE_ASYMPTOTIC;
    out_u2[o] = u2;
    out_tie[o] = tie;
    out_lfc[o] = lfc;
    out_z[o] = num / s;
    out_rbc[o] = 1.0 - (double)u2 / n1n2;
}

static unsigned de_bits_for(int64_t n)
{
    unsigned b = 1;
    while (b < 32 && ((int64_t)1 << b) < n) ++b;
    return b;
}

hipError_t de_temp_bytes(int64_t nnz_max, int64_t keys_max, int64_t n_seg, size_t *bytes)
{
    size_t scan = 0, sort = 0;
    hipError_t e = rocprim::exclusive_scan(nullptr, scan, (const uint32_t *)nullptr, (uint32_t *)nullptr, 0u, (size_t)nnz_max,
                                           rocprim::plus<uint32_t>(), (hipStream_t) nullptr);
    if (e != hipSuccess) return e;
    e = rocprim::radix_sort_keys(nullptr, sort, (const uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)keys_max, 0u,
                                 32u + de_bits_for(n_seg), (hipStream_t) nullptr);
    *bytes = scan > sort ? scan : sort;
    return e;
}

// keys of one matrix's chunk, written from keys[key_base]; cnt / off: [nnz] scratch
hipError_t de_expand_launch(const int32_t *cell, const float *val, int64_t nnz, const int64_t *gptr, int32_t n_genes_chunk,
                            const float *sf, const int64_t *inv_ptr, const int32_t *inv_set, int64_t n_sets, uint32_t *cnt,
                            uint32_t *off, void *temp, size_t temp_bytes, uint64_t *keys, int64_t key_base, hipStream_t st)
{
    if (nnz <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((nnz + 255) / 256);
    hipLaunchKernelGGL(de_count_kernel, dim3(grid), dim3(256), 0, st, cell, nnz, inv_ptr, cnt);
    hipError_t e = rocprim::exclusive_scan(temp, temp_bytes, (const uint32_t *)cnt, off, 0u, (size_t)nnz, rocprim::plus<uint32_t>(), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(de_emit_kernel, dim3(grid), dim3(256), 0, st, cell, val, nnz, gptr, n_genes_chunk, sf, inv_ptr, inv_set,
                       (const uint32_t *)off, n_sets, keys + key_base);
    return hipGetLastError();
}

// keys_a -> keys_b sorted; seg: [n_seg + 1]
hipError_t de_sort_launch(const uint64_t *keys_a, uint64_t *keys_b, int64_t n_keys, int64_t n_seg, void *temp, size_t temp_bytes,
                          int64_t *seg, hipStream_t st)
{
    if (n_keys > 0) {
        hipError_t e = rocprim::radix_sort_keys(temp, temp_bytes, keys_a, keys_b, (size_t)n_keys, 0u, 32u + de_bits_for(n_seg), st);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(de_segptr_kernel, dim3((unsigned)((n_keys + 256) / 256)), dim3(256), 0, st, (const uint64_t *)keys_b, n_keys,
                       n_seg, seg);
    return hipGetLastError();
}

hipError_t de_rank_launch(const uint64_t *keys, const int64_t *seg, int64_t n_sets, const int64_t *set_size, int64_t n_pairs,
                          const int32_t *pair_test, const int32_t *pair_ctrl, int64_t n_genes_chunk, double exp_frac_thresh,
                          double log2_fc_thresh, int32_t *out_status, int64_t *out_i64, double *out_f64, hipStream_t st)
{
    const int64_t n_out = n_genes_chunk * n_pairs;
    if (n_out <= 0) return hipSuccess;
    hipLaunchKernelGGL(de_rank_kernel, dim3((unsigned)n_out), dim3(DE_WAVE), 0, st, keys, seg, n_sets, set_size, n_pairs, pair_test,
                       pair_ctrl, exp_frac_thresh, log2_fc_thresh, out_status, out_i64, out_i64 + n_out, out_i64 + 2 * n_out,
                       out_i64 + 3 * n_out, out_i64 + 4 * n_out, out_f64, out_f64 + n_out, out_f64 + 2 * n_out);
    return hipGetLastError();
}

}  // namespace nabo

// ---- C ABI (include/nabo_de.h) ------------------------------------------------------------------------------------
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/nabo_de.h"
#include "de_exact.h"
#include "host_common.h"

namespace {

using nabo::DevBuf;

constexpr int64_t DE_DEFAULT_BUDGET = (int64_t)2 << 30;
constexpr int64_t DE_MAX_POOLED = (int64_t)1 << 21;      // (n1 + n2)^3 stays inside int64
constexpr int64_t DE_MAX_OUT = (int64_t)1 << 31;         // (gene, pair) results of one chunk: the rank kernel's grid
constexpr int64_t DE_KEY_BYTES = 24;                     // two key buffers and the sort's scratch, per key

thread_local double g_de_ms[3] = {0, 0, 0};
thread_local int64_t g_de_chunks = 0;

struct Csc {
    int64_t n_cells;
    const int64_t *gene_ptr;
    const int32_t *cell;
    const float *val, *sf;
};

// one matrix of the test: the values are the products with the cells' size factors, and only those are checked
int check_csc(const char *which, int64_t n_genes, const Csc &m)
{
    if (m.n_cells < 0 || m.n_cells >= ((int64_t)1 << 31) - 1)
        return nabo::api_fail(NABO_E_INVALID, "%s: n_cells=%lld out of range [0, 2^31 - 1)", which, (long long)m.n_cells);
    return nabo::check_sparse<nabo::SPARSE_SCALED>(which, "gene", "cell", n_genes, m.n_cells, m.gene_ptr, m.cell, m.val, m.sf, false);
}

// cell -> the sets of `role` it is a member of, one entry per membership (CSR by cell)
void invert_sets(int64_t n_cells, int64_t n_sets, const int64_t *set_ptr, const int64_t *members, const std::vector<uint8_t> &role,
                 uint8_t want, std::vector<int64_t> &inv_ptr, std::vector<int32_t> &inv_set)
{
    inv_ptr.assign((size_t)n_cells + 1, 0);
    for (int64_t s = 0; s < n_sets; ++s)
        if (role[s] & want)
            for (int64_t j = set_ptr[s]; j < set_ptr[s + 1]; ++j) ++inv_ptr[members[j] + 1];
    for (int64_t c = 0; c < n_cells; ++c) inv_ptr[c + 1] += inv_ptr[c];
    inv_set.assign((size_t)inv_ptr[n_cells], 0);
    std::vector<int64_t> fill(inv_ptr.begin(), inv_ptr.end() - 1);
    for (int64_t s = 0; s < n_sets; ++s)
        if (role[s] & want)
            for (int64_t j = set_ptr[s]; j < set_ptr[s + 1]; ++j) inv_set[fill[members[j]]++] = (int32_t)s;
}

// resident tables of one matrix and the buffers of its chunk
struct Side {
    Csc m{};
    std::vector<int64_t> inv_ptr, keys_of_gene;          // keys_of_gene[g]: keys gene g emits (prefix sums, [n_genes + 1])
    std::vector<int64_t> gptr;                           // the chunk's column pointers, relative to its first nonzero
    std::vector<int32_t> inv_set;
    DevBuf d_sf, d_inv_ptr, d_inv_set, d_cell, d_val, d_cnt, d_off, d_gptr;
};

int upload_side(Side &s, hipStream_t st)
{
    HIP_TRY(s.d_sf.alloc((size_t)s.m.n_cells * 4));
    HIP_TRY(s.d_inv_ptr.alloc(s.inv_ptr.size() * 8));
    HIP_TRY(s.d_inv_set.alloc(s.inv_set.size() * 4));
    if (s.m.n_cells) HIP_TRY(hipMemcpyAsync(s.d_sf.p, s.m.sf, (size_t)s.m.n_cells * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(s.d_inv_ptr.p, s.inv_ptr.data(), s.inv_ptr.size() * 8, hipMemcpyHostToDevice, st));
    if (!s.inv_set.empty()) HIP_TRY(hipMemcpyAsync(s.d_inv_set.p, s.inv_set.data(), s.inv_set.size() * 4, hipMemcpyHostToDevice, st));
    return NABO_OK;
}

}  // namespace

extern "C" {

int nabo_de_test(int32_t device, int64_t n_genes, int64_t n_cells, const int64_t *gene_ptr, const int32_t *cell, const float *val,
                 const float *sf, int64_t n_cells2, const int64_t *gene_ptr2, const int32_t *cell2, const float *val2, const float *sf2,
                 int64_t n_sets, const int64_t *set_ptr, const int64_t *members, int64_t n_pairs, const int32_t *pair_test,
                 const int32_t *pair_ctrl, double exp_frac_thresh, double log2_fc_thresh, int64_t mem_budget_bytes, int32_t *out_status,
                 int64_t *out_nonzero_test, int64_t *out_n1, int64_t *out_n2, int64_t *out_u2, int64_t *out_tie, double *out_log2_fc,
                 double *out_z, double *out_pval, double *out_rbc)
{
    if (n_genes < 0 || n_genes >= ((int64_t)1 << 31)) return nabo::api_fail(NABO_E_INVALID, "n_genes=%lld out of range", (long long)n_genes);
    if (n_sets < 1 || n_sets >= ((int64_t)1 << 24)) return nabo::api_fail(NABO_E_INVALID, "n_sets=%lld out of range [1, 2^24)", (long long)n_sets);
    int rc = nabo::check_csr_ptr("set_ptr", "set", n_sets, set_ptr);
    if (rc) return rc;
    if (set_ptr[n_sets] > 0 && !members) return nabo::api_fail(NABO_E_INVALID, "members is NULL");
    if (std::isnan(exp_frac_thresh) || std::isnan(log2_fc_thresh)) return nabo::api_fail(NABO_E_INVALID, "a threshold is NaN");
    if (!pair_test) n_pairs = n_sets - 1;
    else if (!pair_ctrl) return nabo::api_fail(NABO_E_INVALID, "pair_ctrl is NULL");
    if (n_pairs < 0 || n_pairs >= ((int64_t)1 << 31)) return nabo::api_fail(NABO_E_INVALID, "n_pairs=%lld out of range", (long long)n_pairs);
    std::vector<int32_t> pt((size_t)n_pairs), pc((size_t)n_pairs);
    for (int64_t p = 0; p < n_pairs; ++p) {
        pt[p] = pair_test ? pair_test[p] : 0;
        pc[p] = pair_test ? pair_ctrl[p] : (int32_t)(p + 1);
        if (pt[p] < 0 || pt[p] >= n_sets || pc[p] < 0 || pc[p] >= n_sets)
            return nabo::api_fail(NABO_E_INVALID, "pair %lld = (%d, %d) names a set outside [0, %lld)", (long long)p, (int)pt[p], (int)pc[p], (long long)n_sets);
    }
    const int64_t n_out = n_genes * n_pairs;
    if (n_out > 0 && (!out_status || !out_nonzero_test || !out_n1 || !out_n2 || !out_u2 || !out_tie || !out_log2_fc || !out_z || !out_pval || !out_rbc))
        return nabo::api_fail(NABO_E_INVALID, "an output array is NULL");
    const bool two = gene_ptr2 != nullptr;
    Side A, B;
    A.m = Csc{n_cells, gene_ptr, cell, val, sf};
    B.m = two ? Csc{n_cells2, gene_ptr2, cell2, val2, sf2} : A.m;
    if ((rc = check_csc("matrix 1", n_genes, A.m))) return rc;
    if (two && (rc = check_csc("matrix 2", n_genes, B.m))) return rc;
    // roles: 1 = test in some pair (reads matrix 1), 2 = control in some pair (reads matrix 2 when there is one)
    std::vector<uint8_t> role((size_t)n_sets, 0);
    for (int64_t p = 0; p < n_pairs; ++p) {
        role[pt[p]] |= 1;
        role[pc[p]] |= 2;
        const int64_t a = set_ptr[pt[p] + 1] - set_ptr[pt[p]], b = set_ptr[pc[p] + 1] - set_ptr[pc[p]];
        if (a == 0) return nabo::api_fail(NABO_E_INVALID, "pair %lld: test set %d is empty", (long long)p, (int)pt[p]);
        if (a + (a < b ? a : b) >= DE_MAX_POOLED)
            return nabo::api_fail(NABO_E_UNSUPPORTED, "pair %lld pools %lld values: fewer than %lld are supported", (long long)p, (long long)(a + (a < b ? a : b)), (long long)DE_MAX_POOLED);
    }
    for (int64_t s = 0; s < n_sets; ++s) {
        if (two && role[s] == 3) return nabo::api_fail(NABO_E_INVALID, "set %lld is test in one pair and control in another, with two matrices", (long long)s);
        const int64_t lim = (two && role[s] == 2) ? n_cells2 : n_cells;
        for (int64_t j = set_ptr[s]; j < set_ptr[s + 1]; ++j)
            if (members[j] < 0 || members[j] >= lim)
                return nabo::api_fail(NABO_E_INVALID, "members[%lld] = %lld is not a cell in [0, %lld)", (long long)j, (long long)members[j], (long long)lim);
    }
    // with one matrix one expansion serves both roles; sets in no pair emit nothing
    for (auto &r : role)
        if (!two && r) r = 3;
    invert_sets(A.m.n_cells, n_sets, set_ptr, members, role, 1, A.inv_ptr, A.inv_set);
    if (two) invert_sets(B.m.n_cells, n_sets, set_ptr, members, role, 2, B.inv_ptr, B.inv_set);
    for (Side *s : {&A, &B}) {
        if (s == &B && !two) break;
        s->keys_of_gene.assign((size_t)n_genes + 1, 0);
        for (int64_t g = 0; g < n_genes; ++g) {
            int64_t k = 0;
            for (int64_t e = s->m.gene_ptr[g]; e < s->m.gene_ptr[g + 1]; ++e) k += s->inv_ptr[s->m.cell[e] + 1] - s->inv_ptr[s->m.cell[e]];
            s->keys_of_gene[g + 1] = s->keys_of_gene[g] + k;
        }
    }
    // chunks of genes within the budget
    const int64_t budget = mem_budget_bytes > 0 ? mem_budget_bytes : DE_DEFAULT_BUDGET;
    const int64_t per_gene_fixed = n_sets * 8 + n_pairs * (4 + 5 * 8 + 3 * 8) + 16;
    auto gene_bytes = [&](int64_t g) {
        int64_t b = per_gene_fixed + (A.m.gene_ptr[g + 1] - A.m.gene_ptr[g]) * 16 + (A.keys_of_gene[g + 1] - A.keys_of_gene[g]) * DE_KEY_BYTES;
        if (two) b += (B.m.gene_ptr[g + 1] - B.m.gene_ptr[g]) * 16 + (B.keys_of_gene[g + 1] - B.keys_of_gene[g]) * DE_KEY_BYTES;
        return b;
    };
    auto keys_in = [&](int64_t g0, int64_t g1) {
        return A.keys_of_gene[g1] - A.keys_of_gene[g0] + (two ? B.keys_of_gene[g1] - B.keys_of_gene[g0] : 0);
    };
    std::vector<int64_t> chunk_start{0};
    int64_t max_genes = 0, max_keys = 0, max_nnz_a = 0, max_nnz_b = 0;
    for (int64_t g = 0, used = 0; g < n_genes; ++g) {
        const int64_t b = gene_bytes(g), g0 = chunk_start.back();
        if (b > budget) return nabo::api_fail(NABO_E_NOMEM, "gene %lld alone needs %lld bytes of device buffers, the budget is %lld", (long long)g, (long long)b, (long long)budget);
        if (g > g0 && (used + b > budget || (g + 1 - g0) * n_sets >= ((int64_t)1 << 31) || (g + 1 - g0) * n_pairs >= DE_MAX_OUT || keys_in(g0, g + 1) >= ((int64_t)1 << 31))) {
            chunk_start.push_back(g);
            used = 0;
        }
        used += b;
    }
    chunk_start.push_back(n_genes);
    for (size_t c = 0; c + 1 < chunk_start.size(); ++c) {
        const int64_t g0 = chunk_start[c], g1 = chunk_start[c + 1];
        if (keys_in(g0, g1) >= ((int64_t)1 << 31)) return nabo::api_fail(NABO_E_UNSUPPORTED, "gene %lld alone emits 2^31 keys or more", (long long)g0);
        max_genes = g1 - g0 > max_genes ? g1 - g0 : max_genes;
        max_keys = keys_in(g0, g1) > max_keys ? keys_in(g0, g1) : max_keys;
        const int64_t na = A.m.gene_ptr[g1] - A.m.gene_ptr[g0], nb = two ? B.m.gene_ptr[g1] - B.m.gene_ptr[g0] : 0;
        max_nnz_a = na > max_nnz_a ? na : max_nnz_a;
        max_nnz_b = nb > max_nnz_b ? nb : max_nnz_b;
    }
    g_de_ms[0] = g_de_ms[1] = g_de_ms[2] = 0;
    g_de_chunks = 0;
    rc = nabo::use_device(device);
    if (rc) return rc;
    if (n_out == 0) return NABO_OK;

    hipStream_t st = nullptr;
    std::vector<int64_t> set_size((size_t)n_sets);
    for (int64_t s = 0; s < n_sets; ++s) set_size[s] = set_ptr[s + 1] - set_ptr[s];
    DevBuf d_size, d_pt, d_pc, d_keys_a, d_keys_b, d_seg, d_temp, d_status, d_i64, d_f64;
    HIP_TRY(d_size.alloc((size_t)n_sets * 8));
    HIP_TRY(d_pt.alloc((size_t)n_pairs * 4));
    HIP_TRY(d_pc.alloc((size_t)n_pairs * 4));
    HIP_TRY(hipMemcpyAsync(d_size.p, set_size.data(), (size_t)n_sets * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_pt.p, pt.data(), (size_t)n_pairs * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_pc.p, pc.data(), (size_t)n_pairs * 4, hipMemcpyHostToDevice, st));
    if ((rc = upload_side(A, st))) return rc;
    if (two && (rc = upload_side(B, st))) return rc;
    const int64_t max_out = max_genes * n_pairs, max_seg = max_genes * n_sets;
    size_t temp_bytes = 0;                                   // the largest scratch any chunk's scan and sort ask for
    for (size_t c = 0; c + 1 < chunk_start.size(); ++c) {
        const int64_t g0 = chunk_start[c], g1 = chunk_start[c + 1];
        const int64_t na = A.m.gene_ptr[g1] - A.m.gene_ptr[g0], nb = two ? B.m.gene_ptr[g1] - B.m.gene_ptr[g0] : 0;
        size_t want = 0;
        HIP_TRY(nabo::de_temp_bytes(na > nb ? na : nb, keys_in(g0, g1), (g1 - g0) * n_sets, &want));
        temp_bytes = want > temp_bytes ? want : temp_bytes;
    }
    HIP_TRY(d_temp.alloc(temp_bytes));
    HIP_TRY(d_keys_a.alloc((size_t)max_keys * 8));
    HIP_TRY(d_keys_b.alloc((size_t)max_keys * 8));
    HIP_TRY(d_seg.alloc((size_t)(max_seg + 1) * 8));
    HIP_TRY(d_status.alloc((size_t)max_out * 4));
    HIP_TRY(d_i64.alloc((size_t)max_out * 5 * 8));
    HIP_TRY(d_f64.alloc((size_t)max_out * 3 * 8));
    for (Side *s : {&A, &B}) {
        if (s == &B && !two) break;
        const int64_t nnz = s == &A ? max_nnz_a : max_nnz_b;
        HIP_TRY(s->d_cell.alloc((size_t)nnz * 4));
        HIP_TRY(s->d_val.alloc((size_t)nnz * 4));
        HIP_TRY(s->d_cnt.alloc((size_t)nnz * 4));
        HIP_TRY(s->d_off.alloc((size_t)nnz * 4));
        HIP_TRY(s->d_gptr.alloc((size_t)(max_genes + 1) * 8));
    }
    nabo::Events<4> E;
    HIP_TRY(E.create());
    std::vector<int64_t> h_i64((size_t)max_out * 5);
    std::vector<double> h_f64((size_t)max_out * 3);

    for (size_t c = 0; c + 1 < chunk_start.size(); ++c) {
        const int64_t g0 = chunk_start[c], g1 = chunk_start[c + 1], ng = g1 - g0;
        if (ng == 0) continue;
        const int64_t nk = keys_in(g0, g1), n_seg = ng * n_sets, no = ng * n_pairs;
        int64_t nnz_side[2] = {0, 0};
        for (Side *s : {&A, &B}) {
            if (s == &B && !two) break;
            const int64_t e0 = s->m.gene_ptr[g0], nnz = s->m.gene_ptr[g1] - e0;
            nnz_side[s == &B] = nnz;
            s->gptr.resize((size_t)ng + 1);
            for (int64_t g = 0; g <= ng; ++g) s->gptr[g] = s->m.gene_ptr[g0 + g] - e0;
            HIP_TRY(hipMemcpyAsync(s->d_gptr.p, s->gptr.data(), (size_t)(ng + 1) * 8, hipMemcpyHostToDevice, st));
            if (nnz) {
                HIP_TRY(hipMemcpyAsync(s->d_cell.p, s->m.cell + e0, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
                HIP_TRY(hipMemcpyAsync(s->d_val.p, s->m.val + e0, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
            }
        }
        HIP_TRY(hipMemsetAsync(d_status.p, 0, (size_t)no * 4, st));
        HIP_TRY(hipMemsetAsync(d_i64.p, 0, (size_t)no * 5 * 8, st));
        HIP_TRY(hipMemsetAsync(d_f64.p, 0, (size_t)no * 3 * 8, st));
        HIP_TRY(hipEventRecord(E.ev[0], st));
        HIP_TRY(nabo::de_expand_launch(A.d_cell.as<int32_t>(), A.d_val.as<float>(), nnz_side[0], A.d_gptr.as<int64_t>(), (int32_t)ng,
                                       A.d_sf.as<float>(), A.d_inv_ptr.as<int64_t>(), A.d_inv_set.as<int32_t>(), n_sets, A.d_cnt.as<uint32_t>(),
                                       A.d_off.as<uint32_t>(), d_temp.p, temp_bytes, d_keys_a.as<uint64_t>(), 0, st));
        if (two)
            HIP_TRY(nabo::de_expand_launch(B.d_cell.as<int32_t>(), B.d_val.as<float>(), nnz_side[1], B.d_gptr.as<int64_t>(), (int32_t)ng,
                                           B.d_sf.as<float>(), B.d_inv_ptr.as<int64_t>(), B.d_inv_set.as<int32_t>(), n_sets, B.d_cnt.as<uint32_t>(),
                                           B.d_off.as<uint32_t>(), d_temp.p, temp_bytes, d_keys_a.as<uint64_t>(),
                                           A.keys_of_gene[g1] - A.keys_of_gene[g0], st));
        HIP_TRY(hipEventRecord(E.ev[1], st));
        HIP_TRY(nabo::de_sort_launch(d_keys_a.as<uint64_t>(), d_keys_b.as<uint64_t>(), nk, n_seg, d_temp.p, temp_bytes, d_seg.as<int64_t>(), st));
        HIP_TRY(hipEventRecord(E.ev[2], st));
        HIP_TRY(nabo::de_rank_launch(d_keys_b.as<uint64_t>(), d_seg.as<int64_t>(), n_sets, d_size.as<int64_t>(), n_pairs, d_pt.as<int32_t>(),
                                     d_pc.as<int32_t>(), ng, exp_frac_thresh, log2_fc_thresh, d_status.as<int32_t>(), d_i64.as<int64_t>(),
                                     d_f64.as<double>(), st));
        HIP_TRY(hipEventRecord(E.ev[3], st));
        HIP_TRY(hipMemcpyAsync(out_status + g0 * n_pairs, d_status.p, (size_t)no * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h_i64.data(), d_i64.p, (size_t)no * 5 * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h_f64.data(), d_f64.p, (size_t)no * 3 * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (int i = 0; i < 3; ++i) HIP_TRY(E.elapsed(i, i + 1, &g_de_ms[i]));
        ++g_de_chunks;
        const size_t o0 = (size_t)(g0 * n_pairs), nb = (size_t)no;
        memcpy(out_nonzero_test + o0, h_i64.data(), nb * 8);
        memcpy(out_n1 + o0, h_i64.data() + nb, nb * 8);
        memcpy(out_n2 + o0, h_i64.data() + 2 * nb, nb * 8);
        memcpy(out_u2 + o0, h_i64.data() + 3 * nb, nb * 8);
        memcpy(out_tie + o0, h_i64.data() + 4 * nb, nb * 8);
        memcpy(out_log2_fc + o0, h_f64.data(), nb * 8);
        memcpy(out_z + o0, h_f64.data() + nb, nb * 8);
        memcpy(out_rbc + o0, h_f64.data() + 2 * nb, nb * 8);
        // p on the host: libm's erfc for the normal approximation, the distribution of U for the small samples
        for (size_t i = o0; i < o0 + nb; ++i) {
            out_pval[i] = 0.0;
            if (out_status[i] == NABO_DE_ASYMPTOTIC) {
                const double p = erfc(out_z[i] * 0.70710678118654752440);
                out_pval[i] = p > 1.0 ? 1.0 : p;
            } else if (out_status[i] == NABO_DE_EXACT) {
                if ((rc = nabo::de_exact_pvalue(out_n1[i], out_n2[i], out_u2[i], &out_pval[i]))) return rc;
            }
        }
    }
    return NABO_OK;
}

int nabo_de_last_device_ms(double ms[3], int64_t *n_chunks)
{
    if (!ms) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    for (int i = 0; i < 3; ++i) ms[i] = g_de_ms[i];
    if (n_chunks) *n_chunks = g_de_chunks;
    return NABO_OK;
}

}  // extern "C"
