// Greedy modularity agglomeration of the reference graph: the kernels of a round's matching and of the cut
// (include/nabo_agglom.h is the contract; nabo/_graph.py:247-264 make_clusters is what it replaces).  The host side, which
// steps the rounds on the levels of the clustering handle, is in community.hip.
//
// Match pass, the hot path.  The gain of the pair {c, d} is D = a_cd 2m - k_c k_d, a signed 128-bit integer, and pairs are
// ordered by D descending, then the lower id, then the higher: a strict total order that both ends of a pair see alike.
// In a pass every free cluster picks the first pair of the order among its free neighbours with D > 0.  A row of a level
// holds each neighbour once, so the pick is a segmented arg-best and needs no table.  Rows go by their length, as in the
// sweep: AG_GROUP lanes share a row of at most `long_threshold` arcs (the sweep's CM_LONG, handed in by the host, which
// also made the level's list of longer rows with it) and meet in a butterfly; a longer row takes a workgroup and a tree in
// LDS.  Rows of clusters that are not free are left alone, so a matched cluster keeps its partner, its D and its arc for
// the rest of the round.  The mark kernel clears `free` at mutual picks; one 64-bit add per wave counts the new pairs.
// The round's pairs are compacted in ascending id and ordered by two stable radix sorts, on the low then the high half of
// D, both complemented (D > 0 here, so the high half is not negative).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "launch.h"

namespace nabo {

constexpr int AG_THREADS = 256;
constexpr int AG_GROUP = 16;   // lanes per row of the short path, as the sweep's CM_GROUP

__device__ __forceinline__ void ag_gain(int64_t a, int64_t two_m, int64_t kc, int64_t kd, int64_t &hi, uint64_t &lo)
{
    const __int128 D = (__int128)a * (__int128)two_m - (__int128)kc * (__int128)kd;
    hi = (int64_t)(D >> 64);
    lo = (uint64_t)D;
}

// pair order: is (D, x, y) before (bD, bx, by)?  x < y and bx < by are the ids of the two pairs; bx < 0: there is no b
__device__ __forceinline__ bool ag_pair_before(int64_t hi, uint64_t lo, int32_t x, int32_t y, int64_t bhi, uint64_t blo, int32_t bx, int32_t by)
{
    if (x < 0) return false;
    if (bx < 0) return true;
    if (hi != bhi) return hi > bhi;
    if (lo != blo) return lo > blo;
    if (x != bx) return x < bx;
    return y < by;
}

// the same seen from row c: partners d and bd (-1: none)
__device__ __forceinline__ bool ag_before(int32_t c, int64_t hi, uint64_t lo, int32_t d, int64_t bhi, uint64_t blo, int32_t bd)
{
    if (d < 0) return false;
    if (bd < 0) return true;
    return ag_pair_before(hi, lo, min(c, d), max(c, d), bhi, blo, min(c, bd), max(c, bd));
}

struct AgPick {
    int64_t hi;
    uint64_t lo;
    int64_t a;
    int32_t d;
};

// arc e of row c against the row's pick so far
__device__ __forceinline__ void ag_try(int32_t c, int64_t kc, int64_t e, const int32_t *__restrict__ nbr, const int64_t *__restrict__ a,
                                       const int64_t *__restrict__ k, const uint8_t *__restrict__ free, int64_t two_m, int any_sign,
                                       AgPick &best)
{
    const int32_t d = nbr[e];
    if (!free[d]) return;
    int64_t hi;
    uint64_t lo;
    const int64_t w = a[e];
    ag_gain(w, two_m, kc, k[d], hi, lo);
    if (!any_sign && !(hi > 0 || (hi == 0 && lo != 0))) return;
    if (ag_before(c, hi, lo, d, best.hi, best.lo, best.d)) best = AgPick{hi, lo, w, d};
}

__global__ __launch_bounds__(AG_THREADS) void ag_pass_short_kernel(int64_t n, const int64_t *__restrict__ ptr, const int32_t *__restrict__ nbr,
                                                                   const int64_t *__restrict__ a, const int64_t *__restrict__ k,
                                                                   const uint8_t *__restrict__ free, int64_t two_m, int long_threshold,
                                                                   int any_sign, int32_t *__restrict__ partner, int64_t *__restrict__ dhi,
                                                                   uint64_t *__restrict__ dlo, int64_t *__restrict__ wa)
{
    constexpr int GROUPS = AG_THREADS / AG_GROUP;
    const int g = threadIdx.x / AG_GROUP, l = threadIdx.x % AG_GROUP;
    const int64_t c = (int64_t)blockIdx.x * GROUPS + g;
    int64_t e0 = 0, kc = 0;
    int len = 0;
    bool mine = false;   // a free row of this path
    if (c < n && free[c]) {
        e0 = ptr[c];
        const int64_t L = ptr[c + 1] - e0;
        mine = L <= long_threshold;
        len = mine ? (int)L : 0;
        kc = k[c];
    }
    AgPick best{0, 0, 0, -1};
    for (int p = l; p < len; p += AG_GROUP) ag_try((int32_t)c, kc, e0 + p, nbr, a, k, free, two_m, any_sign, best);
#pragma unroll
    for (int m = 1; m < AG_GROUP; m <<= 1) {
        AgPick o;
        o.hi = __shfl_xor((long long)best.hi, m, AG_GROUP);
        o.lo = __shfl_xor((unsigned long long)best.lo, m, AG_GROUP);
        o.a = __shfl_xor((long long)best.a, m, AG_GROUP);
        o.d = __shfl_xor(best.d, m, AG_GROUP);
        if (ag_before((int32_t)c, o.hi, o.lo, o.d, best.hi, best.lo, best.d)) best = o;
    }
    if (mine && l == 0) {
        partner[c] = best.d;
        dhi[c] = best.hi;
        dlo[c] = best.lo;
        wa[c] = best.a;
    }
}

__global__ __launch_bounds__(AG_THREADS) void ag_pass_long_kernel(const int32_t *__restrict__ rows, const int64_t *__restrict__ ptr,
                                                                  const int32_t *__restrict__ nbr, const int64_t *__restrict__ a,
                                                                  const int64_t *__restrict__ k, const uint8_t *__restrict__ free, int64_t two_m,
                                                                  int any_sign, int32_t *__restrict__ partner, int64_t *__restrict__ dhi,
                                                                  uint64_t *__restrict__ dlo, int64_t *__restrict__ wa)
{
    __shared__ AgPick s[AG_THREADS];
    const int t = threadIdx.x;
    const int32_t c = rows[blockIdx.x];
    if (!free[c]) return;   // the whole workgroup
    const int64_t e0 = ptr[c], e1 = ptr[c + 1], kc = k[c];
    AgPick best{0, 0, 0, -1};
    for (int64_t e = e0 + t; e < e1; e += AG_THREADS) ag_try(c, kc, e, nbr, a, k, free, two_m, any_sign, best);
    s[t] = best;
    __syncthreads();
    for (int h = AG_THREADS / 2; h > 0; h >>= 1) {
        if (t < h && ag_before(c, s[t + h].hi, s[t + h].lo, s[t + h].d, s[t].hi, s[t].lo, s[t].d)) s[t] = s[t + h];
        __syncthreads();
    }
    if (t == 0) {
        partner[c] = s[0].d;
        dhi[c] = s[0].hi;
        dlo[c] = s[0].lo;
        wa[c] = s[0].a;
    }
}

// c and d are matched iff they picked each other.  Every thread reads and writes the flag of its own cluster only.
__global__ __launch_bounds__(AG_THREADS) void ag_mark_kernel(int64_t n, const int32_t *__restrict__ partner, uint8_t *__restrict__ free,
                                                             unsigned long long *__restrict__ counter)
{
    const int64_t c = (int64_t)blockIdx.x * AG_THREADS + threadIdx.x;
    bool lead = false;
    if (c < n && free[c]) {
        const int32_t p = partner[c];
        if (p >= 0 && partner[p] == (int32_t)c) {
            free[c] = 0;
            lead = c < p;
        }
    }
    const unsigned long long pairs = __ballot(lead);
    if ((threadIdx.x & 63) == 0 && pairs) atomicAdd(counter, (unsigned long long)__popcll(pairs));
}

// flag[c] = c is the lower end of a matched pair
__global__ __launch_bounds__(AG_THREADS) void ag_lead_kernel(int64_t n, const int32_t *__restrict__ partner, const uint8_t *__restrict__ free,
                                                             int32_t *__restrict__ flag)
{
    const int64_t c = (int64_t)blockIdx.x * AG_THREADS + threadIdx.x;
    if (c < n) flag[c] = !free[c] && c < partner[c] ? 1 : 0;
}

// keys[i] = ~half[sel[i]]: ascending complemented = descending
__global__ __launch_bounds__(AG_THREADS) void ag_keys_kernel(int64_t m, const int32_t *__restrict__ sel, const uint64_t *__restrict__ half,
                                                             uint64_t *__restrict__ keys)
{
    const int64_t i = (int64_t)blockIdx.x * AG_THREADS + threadIdx.x;
    if (i < m) keys[i] = ~half[sel[i]];
}

// the first pair of the order over every cluster's pick (one workgroup): sel[0] = its lower end
__global__ __launch_bounds__(AG_THREADS) void ag_first_kernel(int64_t n, const int32_t *__restrict__ partner, const int64_t *__restrict__ dhi,
                                                              const uint64_t *__restrict__ dlo, int32_t *__restrict__ sel)
{
    __shared__ int64_t sh[AG_THREADS];
    __shared__ uint64_t sl[AG_THREADS];
    __shared__ int32_t sx[AG_THREADS], sy[AG_THREADS];
    const int t = threadIdx.x;
    int64_t bhi = 0;
    uint64_t blo = 0;
    int32_t bx = -1, by = -1;
    for (int64_t c = t; c < n; c += AG_THREADS) {
        const int32_t p = partner[c];
        if (p < 0) continue;
        const int32_t x = min((int32_t)c, p), y = max((int32_t)c, p);
        if (ag_pair_before(dhi[c], dlo[c], x, y, bhi, blo, bx, by)) {
            bhi = dhi[c];
            blo = dlo[c];
            bx = x;
            by = y;
        }
    }
    sh[t] = bhi;
    sl[t] = blo;
    sx[t] = bx;
    sy[t] = by;
    __syncthreads();
    for (int h = AG_THREADS / 2; h > 0; h >>= 1) {
        if (t < h && ag_pair_before(sh[t + h], sl[t + h], sx[t + h], sy[t + h], sh[t], sl[t], sx[t], sy[t])) {
            sh[t] = sh[t + h];
            sl[t] = sl[t + h];
            sx[t] = sx[t + h];
            sy[t] = sy[t + h];
        }
        __syncthreads();
    }
    if (t == 0) sel[0] = sx[0];
}

// rec[i] = (rep_a, rep_b, round, a_cd, k_a, k_b); pairs[i] = (c, d) in the level's ids; either may be NULL
__global__ __launch_bounds__(AG_THREADS) void ag_records_kernel(int64_t m, const int32_t *__restrict__ sel, const int32_t *__restrict__ partner,
                                                                const int64_t *__restrict__ wa, const int64_t *__restrict__ k,
                                                                const int32_t *__restrict__ rep, int64_t round, int64_t *__restrict__ rec,
                                                                int32_t *__restrict__ pairs)
{
    const int64_t i = (int64_t)blockIdx.x * AG_THREADS + threadIdx.x;
    if (i >= m) return;
    const int32_t c = sel[i], d = partner[c];
    if (rec) {
        rec[6 * i] = rep[c];
        rec[6 * i + 1] = rep[d];
        rec[6 * i + 2] = round;
        rec[6 * i + 3] = wa[c];
        rec[6 * i + 4] = k[c];
        rec[6 * i + 5] = k[d];
    }
    if (pairs) {
        pairs[2 * i] = c;
        pairs[2 * i + 1] = d;
    }
}

// comm[d] = c for the first `take` pairs (comm is the identity beforehand; every d is met once)
__global__ __launch_bounds__(AG_THREADS) void ag_comm_kernel(int64_t take, const int32_t *__restrict__ sel, const int32_t *__restrict__ partner,
                                                             int32_t *__restrict__ comm)
{
    const int64_t i = (int64_t)blockIdx.x * AG_THREADS + threadIdx.x;
    if (i < take) comm[partner[sel[i]]] = sel[i];
}

// the representatives of the next level: a surviving cluster keeps its own
__global__ __launch_bounds__(AG_THREADS) void ag_rep_kernel(int64_t n, const int32_t *__restrict__ flag, const int32_t *__restrict__ newid,
                                                            const int32_t *__restrict__ rep, int32_t *__restrict__ rep_next)
{
    const int64_t c = (int64_t)blockIdx.x * AG_THREADS + threadIdx.x;
    if (c < n && flag[c]) rep_next[newid[c]] = rep[c];
}

// parent[rep_b] = rep_a for a prefix of the merge list (a cluster is merged away once, so every rep_b is met once)
__global__ __launch_bounds__(AG_THREADS) void ag_parent_kernel(int64_t t, const int32_t *__restrict__ rep_a, const int32_t *__restrict__ rep_b,
                                                               int32_t *__restrict__ parent)
{
    const int64_t i = (int64_t)blockIdx.x * AG_THREADS + threadIdx.x;
    if (i < t) parent[rep_b[i]] = rep_a[i];
}

static inline unsigned ag_grid(int64_t n) { return (unsigned)((n + AG_THREADS - 1) / AG_THREADS); }

int agglom_group() { return AG_GROUP; }

hipError_t agglom_pass_launch(int64_t n, const int64_t *ptr, const int32_t *nbr, const int64_t *a, const int64_t *k, const uint8_t *free,
                              int64_t two_m, int long_threshold, const int32_t *long_rows, int64_t n_long, bool any_sign, int32_t *partner,
                              int64_t *dhi, uint64_t *dlo, int64_t *wa, hipStream_t st)
{
    constexpr int GROUPS = AG_THREADS / AG_GROUP;
    hipLaunchKernelGGL(ag_pass_short_kernel, dim3((unsigned)((n + GROUPS - 1) / GROUPS)), dim3(AG_THREADS), 0, st, n, ptr, nbr, a, k, free, two_m,
                       long_threshold, any_sign ? 1 : 0, partner, dhi, dlo, wa);
    if (n_long > 0)
        hipLaunchKernelGGL(ag_pass_long_kernel, dim3((unsigned)n_long), dim3(AG_THREADS), 0, st, long_rows, ptr, nbr, a, k, free, two_m,
                           any_sign ? 1 : 0, partner, dhi, dlo, wa);
    return hipGetLastError();
}

hipError_t agglom_mark_launch(int64_t n, const int32_t *partner, uint8_t *free, uint64_t *counter, hipStream_t st)
{
    hipLaunchKernelGGL(ag_mark_kernel, dim3(ag_grid(n)), dim3(AG_THREADS), 0, st, n, partner, free, reinterpret_cast<unsigned long long *>(counter));
    return hipGetLastError();
}

hipError_t agglom_first_launch(int64_t n, const int32_t *partner, const int64_t *dhi, const uint64_t *dlo, int32_t *sel, hipStream_t st)
{
    hipLaunchKernelGGL(ag_first_kernel, dim3(1), dim3(AG_THREADS), 0, st, n, partner, dhi, dlo, sel);
    return hipGetLastError();
}

hipError_t agglom_order_temp_bytes(int64_t n, size_t *bytes)
{
    size_t s1 = 0, s2 = 0;
    hipError_t e = rocprim::select(nullptr, s1, rocprim::counting_iterator<int32_t>(0), (const int32_t *)nullptr, (int32_t *)nullptr,
                                   (size_t *)nullptr, (size_t)n, (hipStream_t) nullptr);
    if (e != hipSuccess) return e;
    e = rocprim::radix_sort_pairs(nullptr, s2, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const int32_t *)nullptr, (int32_t *)nullptr,
                                  (size_t)n, 0u, 64u, (hipStream_t) nullptr);
    *bytes = s1 > s2 ? s1 : s2;
    return e;
}

hipError_t agglom_select_launch(int64_t n, const int32_t *partner, const uint8_t *free, int32_t *flag, int32_t *sel, size_t *count, void *temp,
                                size_t temp_bytes, hipStream_t st)
{
    hipLaunchKernelGGL(ag_lead_kernel, dim3(ag_grid(n)), dim3(AG_THREADS), 0, st, n, partner, free, flag);
    return rocprim::select(temp, temp_bytes, rocprim::counting_iterator<int32_t>(0), (const int32_t *)flag, sel, count, (size_t)n, st);
}

hipError_t agglom_sort_launch(int64_t m, const int64_t *dhi, const uint64_t *dlo, int32_t *sel_a, int32_t *sel_b, uint64_t *key_a,
                              uint64_t *key_b, void *temp, size_t temp_bytes, hipStream_t st)
{
    hipLaunchKernelGGL(ag_keys_kernel, dim3(ag_grid(m)), dim3(AG_THREADS), 0, st, m, sel_a, dlo, key_a);
    hipError_t e = rocprim::radix_sort_pairs(temp, temp_bytes, (const uint64_t *)key_a, key_b, (const int32_t *)sel_a, sel_b, (size_t)m, 0u, 64u, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ag_keys_kernel, dim3(ag_grid(m)), dim3(AG_THREADS), 0, st, m, sel_b, reinterpret_cast<const uint64_t *>(dhi), key_a);
    return rocprim::radix_sort_pairs(temp, temp_bytes, (const uint64_t *)key_a, key_b, (const int32_t *)sel_b, sel_a, (size_t)m, 0u, 64u, st);
}

hipError_t agglom_records_launch(int64_t m, const int32_t *sel, const int32_t *partner, const int64_t *wa, const int64_t *k, const int32_t *rep,
                                 int64_t round, int64_t *rec, int32_t *pairs, hipStream_t st)
{
    if (m > 0) hipLaunchKernelGGL(ag_records_kernel, dim3(ag_grid(m)), dim3(AG_THREADS), 0, st, m, sel, partner, wa, k, rep, round, rec, pairs);
    return hipGetLastError();
}

hipError_t agglom_comm_launch(int64_t take, const int32_t *sel, const int32_t *partner, int32_t *comm, hipStream_t st)
{
    if (take > 0) hipLaunchKernelGGL(ag_comm_kernel, dim3(ag_grid(take)), dim3(AG_THREADS), 0, st, take, sel, partner, comm);
    return hipGetLastError();
}

hipError_t agglom_rep_launch(int64_t n, const int32_t *flag, const int32_t *newid, const int32_t *rep, int32_t *rep_next, hipStream_t st)
{
    hipLaunchKernelGGL(ag_rep_kernel, dim3(ag_grid(n)), dim3(AG_THREADS), 0, st, n, flag, newid, rep, rep_next);
    return hipGetLastError();
}

hipError_t agglom_parent_launch(int64_t t, const int32_t *rep_a, const int32_t *rep_b, int32_t *parent, hipStream_t st)
{
    if (t > 0) hipLaunchKernelGGL(ag_parent_kernel, dim3(ag_grid(t)), dim3(AG_THREADS), 0, st, t, rep_a, rep_b, parent);
    return hipGetLastError();
}

}  // namespace nabo
