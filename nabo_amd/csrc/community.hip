// Communities of the reference graph: seeded synchronous Louvain on exact integers, aggregation, the split into
// connected components and the modularity of any labelling (include/nabo_community.h is the contract;
// nabo/_graph.py:266-292 make_leiden_clusters and :415-442 calc_modularity are what it replaces).
//
// Sweep, the hot path.  Every node reads comm, tot and size as they stood at sweep start and writes the other comm
// buffer, so the order in which nodes are visited does not exist.  Rows go to one of three paths by their length:
//   short  (at most CM_LONG arcs): CM_GROUP lanes share a row.  The row's (comm[j], a_ij) pairs are staged in a slice
//          of LDS the group owns; each lane takes the candidates at row positions l, l + CM_GROUP, ... and sums the
//          candidate's weight over the staged row; the lanes' best candidates meet in a butterfly.
//   long   (more arcs): a workgroup per row and a table in LDS keyed by community (open addressing, 32-bit
//          compare-and-swap on the key, 64-bit integer add on the value: exact, hence the same in any order), then a
//          scan of the table for the best score.  A row with more than CM_CAP distinct neighbour communities cannot
//          fit: the workgroup notes the row in a list and leaves it to the third path.
//   huge   (the rows of that list): CM_HUGE_BLOCKS workgroups, each with a dense table of its own in global memory
//          indexed by community, filled with 64-bit integer atomics, read back through the row and cleared again.
// tot and size are integer atomics per node.  Aggregation: flags and a prefix scan renumber the communities, every arc
// becomes a 64-bit key (c_i << 32 | c_j) (inner arcs go to in' by an integer atomic and get the key of a row past the
// last), one radix sort orders them, a segmented sum by key makes the coarse arcs, and the row pointer is read off the
// sorted keys.  The split is min-label propagation over inner arcs with pointer jumping.
//
// The host side of the greedy agglomeration (include/nabo_agglom.h; its kernels are in agglom.hip) is here as well: it
// steps rounds of match passes on the levels of this handle and uses the aggregation, the pointer jumping and the
// numbering by size above.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce_by_key.hpp>
#include <rocprim/device/device_scan.hpp>

#include "../../include/nabo_agglom.h"
#include "../../include/nabo_community.h"
#include "host_common.h"
#include "simple_graph.h"

namespace nabo {

constexpr int CM_THREADS = 256;
constexpr int CM_GROUP = 16;          // lanes per row of the short path
constexpr int CM_LONG = 64;           // rows of more arcs than this take a workgroup
constexpr int CM_CAP_BITS = 11;
constexpr int CM_CAP = 1 << CM_CAP_BITS;   // distinct neighbour communities the LDS table holds
constexpr int CM_HUGE_BLOCKS = 8;     // workgroups (and dense tables) of the third path
constexpr uint64_t CM_GOLD = 0x9E3779B97F4A7C15ull;

__host__ __device__ __forceinline__ uint64_t cm_mix(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// (score, community): larger score first, the lower id on ties
__device__ __forceinline__ bool cm_better(double s, int32_t c, double bs, int32_t bc) { return s > bs || (s == bs && c < bc); }

__device__ __forceinline__ double cm_score(int64_t e, double t, int64_t T) { return __dsub_rn((double)e, __dmul_rn(t, (double)T)); }

// steps 6 - 8 for node i, which has at least one neighbour
__device__ __forceinline__ void cm_decide(int64_t i, int32_t ci, int32_t best_c, double best_s, double score_a,
                                          const int32_t *__restrict__ size, const CommunitySweep &P, int32_t *__restrict__ comm_new,
                                          unsigned long long *__restrict__ counters)
{
    const bool want = best_c != ci && best_s > score_a && !(size[ci] == 1 && size[best_c] == 1 && best_c > ci);
    const bool active = (cm_mix(P.h2 + CM_GOLD * ((uint64_t)i + 1)) >> 63) != 0;
    comm_new[i] = want && active ? best_c : ci;
    if (want) atomicAdd(&counters[1], 1ull);
    if (want && active) atomicAdd(&counters[0], 1ull);
}

__global__ __launch_bounds__(CM_THREADS) void cm_totsize_kernel(int64_t n, const int32_t *__restrict__ comm, const int64_t *__restrict__ k,
                                                                unsigned long long *__restrict__ tot, int32_t *__restrict__ size)
{
    const int64_t i = (int64_t)blockIdx.x * CM_THREADS + threadIdx.x;
    if (i >= n) return;
    const int32_t c = comm[i];
    atomicAdd(&tot[c], (unsigned long long)k[i]);
    atomicAdd(&size[c], 1);
}

__global__ __launch_bounds__(CM_THREADS) void cm_sweep_short_kernel(int64_t n, const int64_t *__restrict__ ptr, const int32_t *__restrict__ nbr,
                                                                    const int64_t *__restrict__ a, const int64_t *__restrict__ k,
                                                                    const int32_t *__restrict__ comm, const int64_t *__restrict__ tot,
                                                                    const int32_t *__restrict__ size, CommunitySweep P,
                                                                    int32_t *__restrict__ comm_new, unsigned long long *__restrict__ counters)
{
    constexpr int GROUPS = CM_THREADS / CM_GROUP;
    __shared__ int32_t s_c[GROUPS][CM_LONG];
    __shared__ int64_t s_a[GROUPS][CM_LONG];
    const int g = threadIdx.x / CM_GROUP, l = threadIdx.x % CM_GROUP;
    const int64_t i = (int64_t)blockIdx.x * GROUPS + g;
    int64_t e0 = 0;
    int len = 0;
    bool mine = false;   // a row of this path with at least one arc
    if (i < n) {
        e0 = ptr[i];
        const int64_t L = ptr[i + 1] - e0;
        if (L == 0 && l == 0) comm_new[i] = comm[i];
        mine = L > 0 && L <= CM_LONG;
        len = mine ? (int)L : 0;
    }
    for (int p = l; p < len; p += CM_GROUP) {
        s_c[g][p] = comm[nbr[e0 + p]];
        s_a[g][p] = a[e0 + p];
    }
    __syncthreads();
    int32_t ci = 0;
    int64_t ki = 0, tot_a = 0;
    double ti = 0.0;
    if (mine) {
        ci = comm[i];
        ki = k[i];
        tot_a = tot[ci] - ki;
        ti = (P.gamma * (double)ki) / P.two_m;
    }
    long long eo = 0;
    for (int p = l; p < len; p += CM_GROUP)
        if (s_c[g][p] == ci) eo += s_a[g][p];
#pragma unroll
    for (int m = 1; m < CM_GROUP; m <<= 1) eo += __shfl_xor(eo, m, CM_GROUP);
    const double score_a = cm_score(eo, ti, tot_a);
    double best_s = score_a;
    int32_t best_c = ci;
    for (int p = l; p < len; p += CM_GROUP) {
        const int32_t c = s_c[g][p];
        if (c == ci) continue;
        int64_t e = 0;
        for (int q = 0; q < len; ++q)
            if (s_c[g][q] == c) e += s_a[g][q];
        const double s = cm_score(e, ti, tot[c]);
        if (cm_better(s, c, best_s, best_c)) {
            best_s = s;
            best_c = c;
        }
    }
#pragma unroll
    for (int m = 1; m < CM_GROUP; m <<= 1) {
        const double os = __shfl_xor(best_s, m, CM_GROUP);
        const int32_t oc = __shfl_xor(best_c, m, CM_GROUP);
        if (cm_better(os, oc, best_s, best_c)) {
            best_s = os;
            best_c = oc;
        }
    }
    if (mine && l == 0) cm_decide(i, ci, best_c, best_s, score_a, size, P, comm_new, counters);
}

// the workgroup's best (score, community) in sS[0], sC[0] on return (all lanes call it)
__device__ __forceinline__ void cm_block_best(double *sS, int32_t *sC, int t, double s, int32_t c)
{
    sS[t] = s;
    sC[t] = c;
    __syncthreads();
    for (int h = CM_THREADS / 2; h > 0; h >>= 1) {
        if (t < h && cm_better(sS[t + h], sC[t + h], sS[t], sC[t])) {
            sS[t] = sS[t + h];
            sC[t] = sC[t + h];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(CM_THREADS) void cm_sweep_long_kernel(const int32_t *__restrict__ rows, const int64_t *__restrict__ ptr,
                                                                   const int32_t *__restrict__ nbr, const int64_t *__restrict__ a,
                                                                   const int64_t *__restrict__ k, const int32_t *__restrict__ comm,
                                                                   const int64_t *__restrict__ tot, const int32_t *__restrict__ size,
                                                                   CommunitySweep P, int32_t *__restrict__ comm_new,
                                                                   unsigned long long *__restrict__ counters, int32_t *__restrict__ ovf,
                                                                   unsigned int *__restrict__ ovf_count)
{
    __shared__ int32_t keys[CM_CAP];
    __shared__ unsigned long long vals[CM_CAP];
    __shared__ double sS[CM_THREADS];
    __shared__ int32_t sC[CM_THREADS];
    __shared__ int s_full;
    __shared__ unsigned long long s_own;
    const int t = threadIdx.x;
    const int64_t i = rows[blockIdx.x];
    const int64_t e0 = ptr[i], e1 = ptr[i + 1];
    for (int s = t; s < CM_CAP; s += CM_THREADS) {
        keys[s] = -1;
        vals[s] = 0;
    }
    if (t == 0) {
        s_full = 0;
        s_own = 0;
    }
    __syncthreads();
    for (int64_t e = e0 + t; e < e1; e += CM_THREADS) {
        const int32_t c = comm[nbr[e]];
        unsigned slot = ((uint32_t)c * 2654435761u) >> (32 - CM_CAP_BITS);
        int probes = 0;
        for (; probes < CM_CAP; ++probes) {
            const int32_t old = atomicCAS(&keys[slot], -1, c);
            if (old == -1 || old == c) {
                atomicAdd(&vals[slot], (unsigned long long)a[e]);
                break;
            }
            slot = (slot + 1) & (CM_CAP - 1);
        }
        if (probes == CM_CAP) s_full = 1;
    }
    __syncthreads();
    if (s_full) {   // more distinct communities than the table holds: the huge path takes the row
        if (t == 0) ovf[atomicAdd(ovf_count, 1u)] = (int32_t)i;
        return;
    }
    const int32_t ci = comm[i];
    const int64_t ki = k[i], tot_a = tot[ci] - ki;
    const double ti = (P.gamma * (double)ki) / P.two_m;
    double best_s = -INFINITY;
    int32_t best_c = INT32_MAX;
    for (int s = t; s < CM_CAP; s += CM_THREADS) {
        const int32_t c = keys[s];
        if (c < 0) continue;
        if (c == ci) {
            s_own = vals[s];
            continue;
        }
        const double sc = cm_score((int64_t)vals[s], ti, tot[c]);
        if (cm_better(sc, c, best_s, best_c)) {
            best_s = sc;
            best_c = c;
        }
    }
    cm_block_best(sS, sC, t, best_s, best_c);
    if (t == 0) {
        const double score_a = cm_score((int64_t)s_own, ti, tot_a);
        best_s = sS[0];
        best_c = sC[0];
        if (cm_better(score_a, ci, best_s, best_c)) {
            best_s = score_a;
            best_c = ci;
        }
        cm_decide(i, ci, best_c, best_s, score_a, size, P, comm_new, counters);
    }
}

// scratch: [gridDim.x][n] of zeros, zeros again on return
__global__ __launch_bounds__(CM_THREADS) void cm_sweep_huge_kernel(int64_t n, const int32_t *__restrict__ ovf, const unsigned int *__restrict__ ovf_count,
                                                                   const int64_t *__restrict__ ptr, const int32_t *__restrict__ nbr,
                                                                   const int64_t *__restrict__ a, const int64_t *__restrict__ k,
                                                                   const int32_t *__restrict__ comm, const int64_t *__restrict__ tot,
                                                                   const int32_t *__restrict__ size, CommunitySweep P,
                                                                   int32_t *__restrict__ comm_new, unsigned long long *__restrict__ counters,
                                                                   unsigned long long *__restrict__ scratch)
{
    __shared__ double sS[CM_THREADS];
    __shared__ int32_t sC[CM_THREADS];
    const int t = threadIdx.x;
    unsigned long long *tab = scratch + (int64_t)blockIdx.x * n;
    const unsigned int cnt = *ovf_count;
    for (unsigned int r = blockIdx.x; r < cnt; r += gridDim.x) {
        const int64_t i = ovf[r];
        const int64_t e0 = ptr[i], e1 = ptr[i + 1];
        for (int64_t e = e0 + t; e < e1; e += CM_THREADS) atomicAdd(&tab[comm[nbr[e]]], (unsigned long long)a[e]);
        __threadfence();
        __syncthreads();
        const int32_t ci = comm[i];
        const int64_t ki = k[i], tot_a = tot[ci] - ki;
        const double ti = (P.gamma * (double)ki) / P.two_m;
        double best_s = -INFINITY;
        int32_t best_c = INT32_MAX;
        for (int64_t e = e0 + t; e < e1; e += CM_THREADS) {
            const int32_t c = comm[nbr[e]];
            if (c == ci) continue;
            const int64_t ec = (int64_t)__hip_atomic_load(&tab[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const double sc = cm_score(ec, ti, tot[c]);
            if (cm_better(sc, c, best_s, best_c)) {
                best_s = sc;
                best_c = c;
            }
        }
        cm_block_best(sS, sC, t, best_s, best_c);
        if (t == 0) {
            const int64_t eo = (int64_t)__hip_atomic_load(&tab[ci], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const double score_a = cm_score(eo, ti, tot_a);
            best_s = sS[0];
            best_c = sC[0];
            if (cm_better(score_a, ci, best_s, best_c)) {
                best_s = score_a;
                best_c = ci;
            }
            cm_decide(i, ci, best_c, best_s, score_a, size, P, comm_new, counters);
        }
        __syncthreads();   // every read of the table is done
        for (int64_t e = e0 + t; e < e1; e += CM_THREADS)
            __hip_atomic_store(&tab[comm[nbr[e]]], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        __syncthreads();
    }
}

__global__ __launch_bounds__(CM_THREADS) void cm_flag_kernel(int64_t n, const int32_t *__restrict__ size, int32_t *__restrict__ flag)
{
    const int64_t i = (int64_t)blockIdx.x * CM_THREADS + threadIdx.x;
    if (i < n) flag[i] = size[i] > 0 ? 1 : 0;
}

// lab[i] = newid[comm[i]]
__global__ __launch_bounds__(CM_THREADS) void cm_relabel_kernel(int64_t n, const int32_t *__restrict__ comm, const int32_t *__restrict__ newid,
                                                                int32_t *__restrict__ lab)
{
    const int64_t i = (int64_t)blockIdx.x * CM_THREADS + threadIdx.x;
    if (i < n) lab[i] = newid[comm[i]];
}

// d[c] += k_i, in2[c] += in_i over the members of c
__global__ __launch_bounds__(CM_THREADS) void cm_part_node_kernel(int64_t n, const int32_t *__restrict__ lab, const int64_t *__restrict__ k,
                                                                  const int64_t *__restrict__ inn, unsigned long long *__restrict__ d,
                                                                  unsigned long long *__restrict__ in2)
{
    const int64_t i = (int64_t)blockIdx.x * CM_THREADS + threadIdx.x;
    if (i >= n) return;
    const int32_t c = lab[i];
    atomicAdd(&d[c], (unsigned long long)k[i]);
    if (inn[i]) atomicAdd(&in2[c], (unsigned long long)inn[i]);
}

// inner arcs go to in2; with keys: every arc's key (c_i << 32 | c_j) and weight, inner arcs the key of row n_next
__global__ __launch_bounds__(CM_THREADS) void cm_part_arc_kernel(int64_t A, const int32_t *__restrict__ src, const int32_t *__restrict__ nbr,
                                                                 const int64_t *__restrict__ a, const int32_t *__restrict__ lab,
                                                                 unsigned long long *__restrict__ in2, int64_t n_next,
                                                                 uint64_t *__restrict__ keys, int64_t *__restrict__ vals)
{
    const int64_t e = (int64_t)blockIdx.x * CM_THREADS + threadIdx.x;
    if (e >= A) return;
    const int32_t ci = lab[src[e]], cj = lab[nbr[e]];
    if (ci == cj) atomicAdd(&in2[ci], (unsigned long long)a[e]);
    if (keys) {
        keys[e] = ci == cj ? (uint64_t)n_next << 32 : ((uint64_t)ci << 32) | (uint64_t)cj;
        vals[e] = ci == cj ? 0 : a[e];
    }
}

__global__ __launch_bounds__(CM_THREADS) void cm_unpack_kernel(const uint64_t *__restrict__ keys, int64_t A, int32_t *__restrict__ src,
                                                               int32_t *__restrict__ nbr)
{
    const int64_t e = (int64_t)blockIdx.x * CM_THREADS + threadIdx.x;
    if (e >= A) return;
    src[e] = (int32_t)(keys[e] >> 32);
    nbr[e] = (int32_t)(keys[e] & 0xFFFFFFFFull);
}

// map[i] = lab[map[i]]
__global__ __launch_bounds__(CM_THREADS) void cm_compose_kernel(int64_t n, int32_t *__restrict__ map, const int32_t *__restrict__ lab)
{
    const int64_t i = (int64_t)blockIdx.x * CM_THREADS + threadIdx.x;
    if (i < n) map[i] = lab[map[i]];
}

// min-label propagation over the arcs inside a part: the lower label is hooked onto the node and onto its label's node
__global__ __launch_bounds__(CM_THREADS) void cm_hook_kernel(int64_t A, const int32_t *__restrict__ src, const int32_t *__restrict__ nbr,
                                                             const int32_t *__restrict__ part, int32_t *__restrict__ lab, int32_t *__restrict__ changed)
{
    const int64_t e = (int64_t)blockIdx.x * CM_THREADS + threadIdx.x;
    if (e >= A) return;
    const int32_t i = src[e], j = nbr[e];
    if (part[i] != part[j]) return;
    const int32_t li = __hip_atomic_load(&lab[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int32_t lj = __hip_atomic_load(&lab[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (lj < li) {
        atomicMin(&lab[li], lj);
        atomicMin(&lab[i], lj);
        *changed = 1;
    }
}

// pointer jumping: lab[i] = the end of the chain i -> lab[i] -> lab[lab[i]] ...  (labels only ever fall, and every
// value met is a node of i's component, so concurrent jumps cannot harm one another)
__global__ __launch_bounds__(CM_THREADS) void cm_jump_kernel(int64_t n, int32_t *__restrict__ lab)
{
    const int64_t i = (int64_t)blockIdx.x * CM_THREADS + threadIdx.x;
    if (i >= n) return;
    int32_t l = __hip_atomic_load(&lab[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (;;) {
        const int32_t ll = __hip_atomic_load(&lab[l], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (ll == l) break;
        l = ll;
    }
    __hip_atomic_store(&lab[i], l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

static inline unsigned cm_grid(int64_t n) { return (unsigned)((n + CM_THREADS - 1) / CM_THREADS); }

int community_huge_blocks() { return CM_HUGE_BLOCKS; }

hipError_t community_totsize_launch(int64_t n, const int32_t *comm, const int64_t *k, int64_t *tot, int32_t *size, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(tot, 0, (size_t)n * 8, st);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(size, 0, (size_t)n * 4, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cm_totsize_kernel, dim3(cm_grid(n)), dim3(CM_THREADS), 0, st, n, comm, k, reinterpret_cast<unsigned long long *>(tot), size);
    return hipGetLastError();
}

hipError_t community_sweep_launch(int64_t n, const int64_t *ptr, const int32_t *nbr, const int64_t *a, const int64_t *k, const int32_t *comm,
                                  const int64_t *tot, const int32_t *size, const CommunitySweep &P, const int32_t *long_rows, int64_t n_long,
                                  int32_t *ovf, unsigned int *ovf_count, int64_t *scratch, int32_t *comm_new, uint64_t *counters,
                                  hipStream_t st)
{
    constexpr int GROUPS = CM_THREADS / CM_GROUP;
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(counters);
    hipLaunchKernelGGL(cm_sweep_short_kernel, dim3((unsigned)((n + GROUPS - 1) / GROUPS)), dim3(CM_THREADS), 0, st, n, ptr, nbr, a, k, comm, tot,
                       size, P, comm_new, cnt);
    if (n_long > 0) {
        hipError_t e = hipMemsetAsync(ovf_count, 0, 4, st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(cm_sweep_long_kernel, dim3((unsigned)n_long), dim3(CM_THREADS), 0, st, long_rows, ptr, nbr, a, k, comm, tot, size, P,
                           comm_new, cnt, ovf, ovf_count);
        hipLaunchKernelGGL(cm_sweep_huge_kernel, dim3(CM_HUGE_BLOCKS), dim3(CM_THREADS), 0, st, n, ovf, ovf_count, ptr, nbr, a, k, comm, tot, size,
                           P, comm_new, cnt, reinterpret_cast<unsigned long long *>(scratch));
    }
    return hipGetLastError();
}

hipError_t community_renumber_temp_bytes(int64_t n, size_t *bytes)
{
    *bytes = 0;
    return rocprim::exclusive_scan(nullptr, *bytes, (const int32_t *)nullptr, (int32_t *)nullptr, 0, (size_t)n, rocprim::plus<int32_t>(),
                                   (hipStream_t) nullptr);
}

hipError_t community_renumber_launch(int64_t n, const int32_t *size, const int32_t *comm, int32_t *flag, int32_t *newid, int32_t *lab, void *temp,
                                     size_t temp_bytes, hipStream_t st)
{
    hipLaunchKernelGGL(cm_flag_kernel, dim3(cm_grid(n)), dim3(CM_THREADS), 0, st, n, size, flag);
    hipError_t e = rocprim::exclusive_scan(temp, temp_bytes, (const int32_t *)flag, newid, 0, (size_t)n, rocprim::plus<int32_t>(), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cm_relabel_kernel, dim3(cm_grid(n)), dim3(CM_THREADS), 0, st, n, comm, newid, lab);
    return hipGetLastError();
}

hipError_t community_part_sums_launch(int64_t n, int64_t A, const int32_t *src, const int32_t *nbr, const int64_t *a, const int64_t *k,
                                      const int64_t *inn, const int32_t *lab, int64_t n_next, int64_t *d, int64_t *in2, uint64_t *keys,
                                      int64_t *vals, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(d, 0, (size_t)n_next * 8, st);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(in2, 0, (size_t)n_next * 8, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cm_part_node_kernel, dim3(cm_grid(n)), dim3(CM_THREADS), 0, st, n, lab, k, inn, reinterpret_cast<unsigned long long *>(d),
                       reinterpret_cast<unsigned long long *>(in2));
    if (A > 0)
        hipLaunchKernelGGL(cm_part_arc_kernel, dim3(cm_grid(A)), dim3(CM_THREADS), 0, st, A, src, nbr, a, lab,
                           reinterpret_cast<unsigned long long *>(in2), n_next, keys, vals);
    return hipGetLastError();
}

hipError_t community_coarse_temp_bytes(int64_t A, int64_t n_next, size_t *bytes)
{
    size_t s1 = 0, s2 = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, s1, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const int64_t *)nullptr,
                                             (int64_t *)nullptr, (size_t)A, 0u, key_sort_bits(n_next), (hipStream_t) nullptr);
    if (e != hipSuccess) return e;
    e = rocprim::reduce_by_key(nullptr, s2, (const uint64_t *)nullptr, (const int64_t *)nullptr, (size_t)A, (uint64_t *)nullptr,
                               (int64_t *)nullptr, (int64_t *)nullptr, rocprim::plus<int64_t>(), rocprim::equal_to<uint64_t>(),
                               (hipStream_t) nullptr);
    *bytes = std::max(s1, s2);
    return e;
}

hipError_t community_coarse_sort_launch(int64_t A, int64_t n_next, const uint64_t *keys_a, const int64_t *vals_a, uint64_t *keys_b,
                                        int64_t *vals_b, uint64_t *ukeys, int64_t *usums, int64_t *n_unique, void *temp, size_t temp_bytes,
                                        hipStream_t st)
{
    hipError_t e = rocprim::radix_sort_pairs(temp, temp_bytes, keys_a, keys_b, vals_a, vals_b, (size_t)A, 0u, key_sort_bits(n_next), st);
    if (e != hipSuccess) return e;
    return rocprim::reduce_by_key(temp, temp_bytes, (const uint64_t *)keys_b, (const int64_t *)vals_b, (size_t)A, ukeys, usums, n_unique,
                                  rocprim::plus<int64_t>(), rocprim::equal_to<uint64_t>(), st);
}

hipError_t community_coarse_arcs_launch(const uint64_t *ukeys, int64_t A, int32_t *src, int32_t *nbr, hipStream_t st)
{
    hipLaunchKernelGGL(cm_unpack_kernel, dim3(cm_grid(A)), dim3(CM_THREADS), 0, st, ukeys, A, src, nbr);
    return hipGetLastError();
}

hipError_t community_compose_launch(int64_t n, int32_t *map, const int32_t *lab, hipStream_t st)
{
    hipLaunchKernelGGL(cm_compose_kernel, dim3(cm_grid(n)), dim3(CM_THREADS), 0, st, n, map, lab);
    return hipGetLastError();
}

hipError_t community_hook_launch(int64_t n, int64_t A, const int32_t *src, const int32_t *nbr, const int32_t *part, int32_t *lab,
                                 int32_t *changed, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(changed, 0, 4, st);
    if (e != hipSuccess) return e;
    if (A > 0) {
        hipLaunchKernelGGL(cm_hook_kernel, dim3(cm_grid(A)), dim3(CM_THREADS), 0, st, A, src, nbr, part, lab, changed);
        hipLaunchKernelGGL(cm_jump_kernel, dim3(cm_grid(n)), dim3(CM_THREADS), 0, st, n, lab);
    }
    return hipGetLastError();
}

hipError_t community_jump_launch(int64_t n, int32_t *lab, hipStream_t st)
{
    hipLaunchKernelGGL(cm_jump_kernel, dim3(cm_grid(n)), dim3(CM_THREADS), 0, st, n, lab);
    return hipGetLastError();
}

}  // namespace nabo

using nabo::DevBuf;

namespace {

struct Level {
    int64_t n = 0, A = 0, n_long = 0;
    DevBuf ptr, src, nbr, a, k, inn, long_rows, ovf, scratch;
};

struct Record {
    int64_t n, n_next, sweeps, moved;
    double q;
};

typedef unsigned __int128 u128;

double modularity_of(u128 sum_in, u128 sum_d2, int64_t two_m, double gamma)
{
    if (two_m == 0) return 0.0;
    const double m2 = (double)two_m;
    const double lhs = (double)sum_in / m2;
    const double rhs = gamma * ((double)sum_d2 / (m2 * m2));
    return lhs - rhs;
}

// the state of the agglomeration (include/nabo_agglom.h): the buffers of a round, sized by n0 at the first use, and the
// dendrogram of the last run
struct Agglom {
    DevBuf free, partner, dhi, dlo, wa, sel[2], key[2], rec, pairs, rep[2], counters, count;
    int rep_cur = 0;
    bool ran = false;
    int64_t rounds = 0, passes = 0, peak = 0, n_end = 0;
    std::vector<int64_t> merges;   // 6 per merge
    std::vector<double> q_path;
    double ms[4] = {0, 0, 0, 0};
};

}  // namespace

struct nabo_community {
    int device = 0;
    int64_t n0 = 0, two_m = 0;
    double gamma = 1.0;
    uint64_t seed = 4466;
    int max_sweeps = 128, max_levels = 32, split = 1;
    Level lv0;
    std::unique_ptr<Level> coarse;   // the current level when it is not level 0
    int cur = 0;                     // which of comm[2] holds the current level's comm
    DevBuf comm[2], tot, size, counters, ovf_count, map0, flag, newid, lab, d, in2, changed, temp, keys_a, keys_b, vals_a, vals_b, ukeys,
        usums, n_unique;
    std::vector<int64_t> h_k0, h_in0;
    bool ran = false;
    std::vector<int32_t> labels;
    int32_t n_clusters = 0;
    double q = 0.0;
    std::vector<Record> history;
    hipEvent_t ev[2] = {};
    double ms[4] = {0, 0, 0, 0};
    Agglom ag;
    ~nabo_community()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    Level &level() { return coarse ? *coarse : lv0; }
};

namespace {

// the list of long rows of a level and what the huge path needs for them
int level_long_rows(Level &lv, const std::vector<int64_t> &ptr)
{
    const std::vector<int32_t> rows = nabo::long_rows(ptr, nabo::CM_LONG);
    lv.n_long = (int64_t)rows.size();
    if (rows.empty()) return NABO_OK;
    HIP_TRY(lv.long_rows.alloc(rows.size() * 4));
    HIP_TRY(lv.ovf.alloc(rows.size() * 4));
    HIP_TRY(lv.scratch.alloc((size_t)nabo::community_huge_blocks() * (size_t)lv.n * 8));
    HIP_TRY(hipMemcpy(lv.long_rows.p, rows.data(), rows.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(lv.scratch.p, 0, (size_t)nabo::community_huge_blocks() * (size_t)lv.n * 8));
    return NABO_OK;
}

int community_identity(nabo_community *H)
{
    H->cur = 0;
    HIP_TRY(nabo::iota_launch(H->comm[0].as<uint32_t>(), H->level().n, nullptr));
    return NABO_OK;
}

int community_rewind(nabo_community *H)
{
    H->coarse.reset();
    HIP_TRY(nabo::iota_launch(H->map0.as<uint32_t>(), H->n0, nullptr));
    int rc = community_identity(H);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return NABO_OK;
}

int community_create(nabo_community *H, int64_t n, const int64_t *ptr, const int64_t *nbr, const double *w, double scale)
{
    // the simple graph (simple_graph.h) of the pairs whose weight does not quantise to 0
    nabo::SimpleGraph g;
    nabo::simple_pairs(g, n, ptr, nbr, true);
    std::vector<int64_t> qw(g.pairs.size());
    for (size_t p = 0; p < qw.size(); ++p) {
        const double wp = w[g.last[p]], q = std::rint(wp * scale);
        if (!(q <= 2147483648.0))
            return nabo::api_fail(NABO_E_INVALID, "w[%lld] = %g quantises to %g, above 2^31", (long long)g.last[p], wp, q);
        qw[p] = (int64_t)q;
    }
    std::vector<int64_t> k((size_t)n, 0), inn((size_t)n, 0);
    u128 two_m = 0;
    nabo::simple_rows(g, n, [&](size_t p) { return qw[p] != 0; }, [&](size_t p, int64_t a, int64_t b) {
        two_m += 2 * (u128)qw[p];
        k[(size_t)a] += qw[p];
        k[(size_t)b] += qw[p];
        if (a == b) inn[(size_t)a] = qw[p];
    });
    if (two_m >= ((u128)1 << 53)) return nabo::api_fail(NABO_E_INVALID, "the quantised weights add up to 2m >= 2^53: lower weight_scale");
    const std::vector<int64_t> &rptr = g.rptr;
    const std::vector<int32_t> &rnbr = g.rnbr;
    const int64_t A = rptr[(size_t)n];
    std::vector<int32_t> rsrc((size_t)A);
    std::vector<int64_t> ra((size_t)A);
    for (int64_t i = 0; i < n; ++i)
        for (int64_t e = rptr[(size_t)i]; e < rptr[(size_t)i + 1]; ++e) {
            rsrc[(size_t)e] = (int32_t)i;
            ra[(size_t)e] = qw[(size_t)g.slot_pair[(size_t)e]];
        }
    H->n0 = n;
    H->two_m = (int64_t)two_m;
    H->h_k0 = k;
    H->h_in0 = inn;
    Level &lv = H->lv0;
    lv.n = n;
    lv.A = A;
    const size_t nb = (size_t)n * 8;
    HIP_TRY(lv.ptr.alloc(nb + 8));
    HIP_TRY(lv.k.alloc(nb));
    HIP_TRY(lv.inn.alloc(nb));
    HIP_TRY(lv.src.alloc((size_t)A * 4));
    HIP_TRY(lv.nbr.alloc((size_t)A * 4));
    HIP_TRY(lv.a.alloc((size_t)A * 8));
    HIP_TRY(hipMemcpy(lv.ptr.p, rptr.data(), nb + 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(lv.k.p, k.data(), nb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(lv.inn.p, inn.data(), nb, hipMemcpyHostToDevice));
    if (A) {
        HIP_TRY(hipMemcpy(lv.src.p, rsrc.data(), (size_t)A * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(lv.nbr.p, rnbr.data(), (size_t)A * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(lv.a.p, ra.data(), (size_t)A * 8, hipMemcpyHostToDevice));
    }
    int rc = level_long_rows(lv, rptr);
    if (rc) return rc;
    for (DevBuf *b : {&H->comm[0], &H->comm[1], &H->size, &H->map0, &H->flag, &H->newid, &H->lab}) HIP_TRY(b->alloc((size_t)n * 4));
    for (DevBuf *b : {&H->tot, &H->d, &H->in2}) HIP_TRY(b->alloc(nb));
    HIP_TRY(H->ovf_count.alloc(4));
    HIP_TRY(H->changed.alloc(4));
    HIP_TRY(H->n_unique.alloc(8));
    for (DevBuf *b : {&H->keys_a, &H->keys_b, &H->vals_a, &H->vals_b, &H->ukeys, &H->usums}) HIP_TRY(b->alloc((size_t)A * 8));
    for (hipEvent_t &e : H->ev) HIP_TRY(hipEventCreate(&e));
    return community_rewind(H);
}

// one sweep of the current level, queued; counters: {moved, want} of this sweep, zero beforehand
int community_sweep_enqueue(nabo_community *H, int64_t level, int64_t sweep, uint64_t *counters)
{
    Level &lv = H->level();
    nabo::CommunitySweep P;
    P.gamma = H->gamma;
    P.two_m = (double)H->two_m;
    const uint64_t h1 = nabo::cm_mix(H->seed + nabo::CM_GOLD * ((uint64_t)level + 1));
    P.h2 = nabo::cm_mix(h1 + nabo::CM_GOLD * ((uint64_t)sweep + 1));
    const int32_t *comm = H->comm[H->cur].as<int32_t>();
    HIP_TRY(nabo::community_totsize_launch(lv.n, comm, lv.k.as<int64_t>(), H->tot.as<int64_t>(), H->size.as<int32_t>(), nullptr));
    HIP_TRY(nabo::community_sweep_launch(lv.n, lv.ptr.as<int64_t>(), lv.nbr.as<int32_t>(), lv.a.as<int64_t>(), lv.k.as<int64_t>(), comm,
                                         H->tot.as<int64_t>(), H->size.as<int32_t>(), P, lv.long_rows.as<int32_t>(), lv.n_long,
                                         lv.ovf.as<int32_t>(), H->ovf_count.as<unsigned int>(), lv.scratch.as<int64_t>(),
                                         H->comm[H->cur ^ 1].as<int32_t>(), counters, nullptr));
    H->cur ^= 1;
    return NABO_OK;
}

constexpr int CM_BATCH = 4;   // sweeps queued between two reads of `want` (a sweep after want == 0 changes nothing)

int community_phase(nabo_community *H, int64_t level, int64_t *sweeps, int64_t *moved)
{
    const size_t cb = (size_t)H->max_sweeps * 16;
    int rc = H->counters.reserve(cb);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(H->counters.p, 0, cb, nullptr));
    uint64_t *cnt = H->counters.as<uint64_t>();
    *sweeps = 0;
    *moved = 0;
    uint64_t h[2 * CM_BATCH];
    for (int s = 0; s < H->max_sweeps;) {
        const int batch = std::min(CM_BATCH, H->max_sweeps - s);
        for (int b = 0; b < batch; ++b) {
            rc = community_sweep_enqueue(H, level, s + b, cnt + 2 * (s + b));
            if (rc) return rc;
        }
        HIP_TRY(hipMemcpy(h, cnt + 2 * s, (size_t)batch * 16, hipMemcpyDeviceToHost));
        for (int b = 0; b < batch; ++b) {
            *moved += (int64_t)h[2 * b];
            *sweeps = s + b + 1;
            if (h[2 * b + 1] == 0) return NABO_OK;
        }
        s += batch;
    }
    return NABO_OK;
}

// aggregates the current level by its comm; *out_in, *out_d2: the sums the modularity of the new partition needs
int community_aggregate(nabo_community *H, u128 *out_in, u128 *out_d2)
{
    Level &lv = H->level();
    hipStream_t st = nullptr;
    const int64_t n = lv.n, A = lv.A;
    const int32_t *comm = H->comm[H->cur].as<int32_t>();
    HIP_TRY(nabo::community_totsize_launch(n, comm, lv.k.as<int64_t>(), H->tot.as<int64_t>(), H->size.as<int32_t>(), st));
    size_t tb = 0;
    HIP_TRY(nabo::community_renumber_temp_bytes(n, &tb));
    int rc = H->temp.reserve(tb);
    if (rc) return rc;
    HIP_TRY(nabo::community_renumber_launch(n, H->size.as<int32_t>(), comm, H->flag.as<int32_t>(), H->newid.as<int32_t>(), H->lab.as<int32_t>(),
                                            H->temp.p, tb, st));
    int32_t last[2];
    HIP_TRY(hipMemcpy(&last[0], H->newid.as<int32_t>() + (n - 1), 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&last[1], H->flag.as<int32_t>() + (n - 1), 4, hipMemcpyDeviceToHost));
    const int64_t n2 = (int64_t)last[0] + last[1];
    if (n2 < 1 || n2 > n) return nabo::api_fail(NABO_E_HIP, "the renumbering returned %lld communities for %lld nodes", (long long)n2, (long long)n);
    std::unique_ptr<Level> nx(new Level);
    nx->n = n2;
    HIP_TRY(nx->ptr.alloc((size_t)n2 * 8 + 8));
    HIP_TRY(nx->k.alloc((size_t)n2 * 8));
    HIP_TRY(nx->inn.alloc((size_t)n2 * 8));
    HIP_TRY(nabo::community_part_sums_launch(n, A, lv.src.as<int32_t>(), lv.nbr.as<int32_t>(), lv.a.as<int64_t>(), lv.k.as<int64_t>(),
                                             lv.inn.as<int64_t>(), H->lab.as<int32_t>(), n2, nx->k.as<int64_t>(), nx->inn.as<int64_t>(),
                                             H->keys_a.as<uint64_t>(), H->vals_a.as<int64_t>(), st));
    int64_t A2 = 0;
    if (A > 0) {
        HIP_TRY(nabo::community_coarse_temp_bytes(A, n2, &tb));
        if ((rc = H->temp.reserve(tb))) return rc;
        HIP_TRY(nabo::community_coarse_sort_launch(A, n2, H->keys_a.as<uint64_t>(), H->vals_a.as<int64_t>(), H->keys_b.as<uint64_t>(),
                                                   H->vals_b.as<int64_t>(), H->ukeys.as<uint64_t>(), H->usums.as<int64_t>(),
                                                   H->n_unique.as<int64_t>(), H->temp.p, tb, st));
        int64_t nu = 0;
        HIP_TRY(hipMemcpy(&nu, H->n_unique.p, 8, hipMemcpyDeviceToHost));
        if (nu < 1 || nu > A) return nabo::api_fail(NABO_E_HIP, "the coarse graph has %lld keys for %lld arcs", (long long)nu, (long long)A);
        HIP_TRY(nabo::key_rowptr_launch(H->ukeys.as<uint64_t>(), nu, n2, nx->ptr.as<int64_t>(), st));
        HIP_TRY(hipMemcpy(&A2, nx->ptr.as<int64_t>() + n2, 8, hipMemcpyDeviceToHost));
        if (A2 < 0 || A2 > nu) return nabo::api_fail(NABO_E_HIP, "the coarse graph has %lld arcs for %lld keys", (long long)A2, (long long)nu);
    } else
        HIP_TRY(hipMemset(nx->ptr.p, 0, (size_t)n2 * 8 + 8));
    nx->A = A2;
    HIP_TRY(nx->src.alloc((size_t)A2 * 4));
    HIP_TRY(nx->nbr.alloc((size_t)A2 * 4));
    HIP_TRY(nx->a.alloc((size_t)A2 * 8));
    if (A2 > 0) {
        HIP_TRY(nabo::community_coarse_arcs_launch(H->ukeys.as<uint64_t>(), A2, nx->src.as<int32_t>(), nx->nbr.as<int32_t>(), st));
        HIP_TRY(hipMemcpyAsync(nx->a.p, H->usums.p, (size_t)A2 * 8, hipMemcpyDeviceToDevice, st));
    }
    HIP_TRY(nabo::community_compose_launch(H->n0, H->map0.as<int32_t>(), H->lab.as<int32_t>(), st));
    std::vector<int64_t> hp((size_t)n2 + 1), hk((size_t)n2), hi((size_t)n2);
    HIP_TRY(hipMemcpy(hp.data(), nx->ptr.p, (size_t)n2 * 8 + 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(hk.data(), nx->k.p, (size_t)n2 * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(hi.data(), nx->inn.p, (size_t)n2 * 8, hipMemcpyDeviceToHost));
    u128 si = 0, sd = 0;
    for (int64_t c = 0; c < n2; ++c) {
        si += (u128)hi[(size_t)c];
        sd += (u128)hk[(size_t)c] * (u128)hk[(size_t)c];
    }
    if (out_in) *out_in = si;
    if (out_d2) *out_d2 = sd;
    rc = level_long_rows(*nx, hp);
    if (rc) return rc;
    H->coarse = std::move(nx);
    return community_identity(H);
}

// the sums of a labelling of the level-0 nodes; dense: device labels in [0, C)
int community_label_sums(nabo_community *H, const int32_t *dense, int64_t C, u128 *sum_in, u128 *sum_d2)
{
    Level &lv = H->lv0;
    HIP_TRY(nabo::community_part_sums_launch(lv.n, lv.A, lv.src.as<int32_t>(), lv.nbr.as<int32_t>(), lv.a.as<int64_t>(), lv.k.as<int64_t>(),
                                             lv.inn.as<int64_t>(), dense, C, H->d.as<int64_t>(), H->in2.as<int64_t>(), nullptr, nullptr, nullptr));
    std::vector<int64_t> hd((size_t)C), hi((size_t)C);
    HIP_TRY(hipMemcpy(hd.data(), H->d.p, (size_t)C * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(hi.data(), H->in2.p, (size_t)C * 8, hipMemcpyDeviceToHost));
    *sum_in = 0;
    *sum_d2 = 0;
    for (int64_t c = 0; c < C; ++c) {
        *sum_in += (u128)hi[(size_t)c];
        *sum_d2 += (u128)hd[(size_t)c] * (u128)hd[(size_t)c];
    }
    return NABO_OK;
}

// any labels -> dense ids 0 .. C-1 in ascending label
int64_t dense_labels(const int32_t *labels, int64_t n, std::vector<int32_t> &dense)
{
    std::vector<int32_t> u(labels, labels + n);
    std::sort(u.begin(), u.end());
    u.erase(std::unique(u.begin(), u.end()), u.end());
    dense.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) dense[(size_t)i] = (int32_t)(std::lower_bound(u.begin(), u.end(), labels[i]) - u.begin());
    return (int64_t)u.size();
}

// the result step: part [n0] (any values) -> out in 1 .. C by size
int community_finish(nabo_community *H, const int32_t *part, int split, std::vector<int32_t> &out, int32_t *n_clusters)
{
    const int64_t n = H->n0;
    Level &lv = H->lv0;
    std::vector<int32_t> comp(part, part + n);
    if (split) {
        HIP_TRY(hipMemcpy(H->flag.p, part, (size_t)n * 4, hipMemcpyHostToDevice));   // flag: the part of each node
        HIP_TRY(nabo::iota_launch(H->lab.as<uint32_t>(), n, nullptr));
        for (int64_t it = 0;; ++it) {
            if (it > n) return nabo::api_fail(NABO_E_HIP, "the component split did not settle");
            HIP_TRY(nabo::community_hook_launch(n, lv.A, lv.src.as<int32_t>(), lv.nbr.as<int32_t>(), H->flag.as<int32_t>(), H->lab.as<int32_t>(),
                                                H->changed.as<int32_t>(), nullptr));
            int32_t ch = 0;
            HIP_TRY(hipMemcpy(&ch, H->changed.p, 4, hipMemcpyDeviceToHost));
            if (!ch) break;
        }
        HIP_TRY(hipMemcpy(comp.data(), H->lab.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    }
    // 1 .. C by descending node count, ties by smallest member id
    std::vector<int32_t> dense;
    const int64_t C = dense_labels(comp.data(), n, dense);
    std::vector<int64_t> cnt((size_t)C, 0), first((size_t)C, -1);
    for (int64_t i = 0; i < n; ++i) {
        ++cnt[(size_t)dense[(size_t)i]];
        if (first[(size_t)dense[(size_t)i]] < 0) first[(size_t)dense[(size_t)i]] = i;
    }
    std::vector<int32_t> order((size_t)C), rank((size_t)C);
    for (int64_t c = 0; c < C; ++c) order[(size_t)c] = (int32_t)c;
    std::sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {
        if (cnt[(size_t)x] != cnt[(size_t)y]) return cnt[(size_t)x] > cnt[(size_t)y];
        return first[(size_t)x] < first[(size_t)y];
    });
    for (int64_t r = 0; r < C; ++r) rank[(size_t)order[(size_t)r]] = (int32_t)r;
    out.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) out[(size_t)i] = rank[(size_t)dense[(size_t)i]] + 1;
    *n_clusters = (int32_t)C;
    return NABO_OK;
}

int community_modularity(nabo_community *H, const int32_t *labels, double gamma, double *q)
{
    std::vector<int32_t> dense;
    const int64_t C = dense_labels(labels, H->n0, dense);
    HIP_TRY(hipMemcpy(H->newid.p, dense.data(), (size_t)H->n0 * 4, hipMemcpyHostToDevice));
    u128 si, sd;
    int rc = community_label_sums(H, H->newid.as<int32_t>(), C, &si, &sd);
    if (rc) return rc;
    *q = modularity_of(si, sd, H->two_m, gamma);
    return NABO_OK;
}

int community_run(nabo_community *H)
{
    H->ran = false;
    H->history.clear();
    for (double &m : H->ms) m = 0;
    int rc = community_rewind(H);
    if (rc) return rc;
    nabo::PhaseTimer T{H->ev, H->ms, 3};
    const int64_t n = H->n0;
    u128 si = 0, sd = 0;
    for (int64_t i = 0; i < n; ++i) {
        si += (u128)H->h_in0[(size_t)i];
        sd += (u128)H->h_k0[(size_t)i] * (u128)H->h_k0[(size_t)i];
    }
    double best_q = modularity_of(si, sd, H->two_m, H->gamma), cur_q = best_q;
    std::vector<int32_t> best((size_t)n);
    for (int64_t i = 0; i < n; ++i) best[(size_t)i] = (int32_t)i;
    for (int level = 0; level < H->max_levels; ++level) {
        int64_t sweeps = 0, moved = 0;
        const int64_t n_level = H->level().n;
        if ((rc = T.start())) return rc;
        if ((rc = community_phase(H, level, &sweeps, &moved))) return rc;
        if ((rc = T.stop(0))) return rc;
        if (moved == 0) {
            H->history.push_back(Record{n_level, n_level, sweeps, 0, cur_q});
            break;
        }
        if ((rc = T.start())) return rc;
        if ((rc = community_aggregate(H, &si, &sd))) return rc;
        if ((rc = T.stop(1))) return rc;
        cur_q = modularity_of(si, sd, H->two_m, H->gamma);
        H->history.push_back(Record{n_level, H->level().n, sweeps, moved, cur_q});
        if (cur_q > best_q) {
            best_q = cur_q;
            HIP_TRY(hipMemcpy(best.data(), H->map0.p, (size_t)n * 4, hipMemcpyDeviceToHost));
        }
    }
    if ((rc = T.start())) return rc;
    if ((rc = community_finish(H, best.data(), H->split, H->labels, &H->n_clusters))) return rc;
    if ((rc = community_modularity(H, H->labels.data(), H->gamma, &H->q))) return rc;
    if ((rc = T.stop(2))) return rc;
    H->ran = true;
    return NABO_OK;
}

// ---- the agglomeration (include/nabo_agglom.h) ----------------------------------------------------------------------

constexpr int AG_BATCH = 4;   // passes queued between two reads of the pair counters (a pass after an empty one changes nothing)

int agglom_reserve(nabo_community *H)
{
    Agglom &G = H->ag;
    const size_t n = (size_t)H->n0, half = n / 2 + 1;
    int rc;
    for (DevBuf *b : {&G.partner, &G.sel[0], &G.sel[1], &G.rep[0], &G.rep[1]})
        if ((rc = b->reserve(n * 4))) return rc;
    for (DevBuf *b : {&G.dhi, &G.dlo, &G.wa, &G.key[0], &G.key[1], &G.pairs})
        if ((rc = b->reserve(n * 8))) return rc;
    if ((rc = G.free.reserve(n))) return rc;
    if ((rc = G.rec.reserve(half * 48))) return rc;
    if ((rc = G.counters.reserve(AG_BATCH * 8))) return rc;
    return G.count.reserve(8);
}

int agglom_pass_enqueue(nabo_community *H, bool any_sign, int32_t *partner, int64_t *dhi, uint64_t *dlo, int64_t *wa)
{
    Level &lv = H->level();
    HIP_TRY(nabo::agglom_pass_launch(lv.n, lv.ptr.as<int64_t>(), lv.nbr.as<int32_t>(), lv.a.as<int64_t>(), lv.k.as<int64_t>(),
                                     H->ag.free.as<uint8_t>(), H->two_m, nabo::CM_LONG, lv.long_rows.as<int32_t>(), lv.n_long, any_sign, partner,
                                     dhi, dlo, wa, nullptr));
    return NABO_OK;
}

// one round's matching on the current level: the lower ends of its pairs in pair order in ag.sel[0], the other ends in
// ag.partner.  T (may be NULL): the passes go to ms[0], the ordering to ms[1]
int agglom_round(nabo_community *H, int64_t *n_pairs, int64_t *passes, nabo::PhaseTimer *T)
{
    Agglom &G = H->ag;
    Level &lv = H->level();
    const int64_t n = lv.n;
    int rc;
    *n_pairs = 0;
    *passes = 0;
    if (T && (rc = T->start())) return rc;
    HIP_TRY(hipMemsetAsync(G.free.p, 1, (size_t)n, nullptr));
    HIP_TRY(hipMemsetAsync(G.partner.p, 0xFF, (size_t)n * 4, nullptr));
    for (bool done = false; !done;) {
        if (*passes > n) return nabo::api_fail(NABO_E_HIP, "the matching did not settle in %lld passes", (long long)*passes);
        HIP_TRY(hipMemsetAsync(G.counters.p, 0, AG_BATCH * 8, nullptr));
        for (int b = 0; b < AG_BATCH; ++b) {
            if ((rc = agglom_pass_enqueue(H, false, G.partner.as<int32_t>(), G.dhi.as<int64_t>(), G.dlo.as<uint64_t>(), G.wa.as<int64_t>())))
                return rc;
            HIP_TRY(nabo::agglom_mark_launch(n, G.partner.as<int32_t>(), G.free.as<uint8_t>(), G.counters.as<uint64_t>() + b, nullptr));
        }
        uint64_t h[AG_BATCH];
        HIP_TRY(hipMemcpy(h, G.counters.p, AG_BATCH * 8, hipMemcpyDeviceToHost));
        for (int b = 0; b < AG_BATCH && !done; ++b) {
            ++*passes;
            *n_pairs += (int64_t)h[b];
            done = h[b] == 0;
        }
    }
    if (T && (rc = T->stop(0))) return rc;
    if (*n_pairs > n / 2) return nabo::api_fail(NABO_E_HIP, "the matching returned %lld pairs for %lld clusters", (long long)*n_pairs, (long long)n);
    if (T && (rc = T->start())) return rc;
    if (*n_pairs == 0 && lv.A > 0) {   // no positive gain: the first pair of the order, whatever its sign
        if ((rc = agglom_pass_enqueue(H, true, G.partner.as<int32_t>(), G.dhi.as<int64_t>(), G.dlo.as<uint64_t>(), G.wa.as<int64_t>()))) return rc;
        HIP_TRY(nabo::agglom_first_launch(n, G.partner.as<int32_t>(), G.dhi.as<int64_t>(), G.dlo.as<uint64_t>(), G.sel[0].as<int32_t>(), nullptr));
        *n_pairs = 1;
    } else if (*n_pairs > 0) {
        size_t tb = 0;
        HIP_TRY(nabo::agglom_order_temp_bytes(n, &tb));
        if ((rc = H->temp.reserve(tb))) return rc;
        HIP_TRY(nabo::agglom_select_launch(n, G.partner.as<int32_t>(), G.free.as<uint8_t>(), H->flag.as<int32_t>(), G.sel[0].as<int32_t>(),
                                           G.count.as<size_t>(), H->temp.p, tb, nullptr));
        size_t cnt = 0;
        HIP_TRY(hipMemcpy(&cnt, G.count.p, sizeof cnt, hipMemcpyDeviceToHost));
        if ((int64_t)cnt != *n_pairs)
            return nabo::api_fail(NABO_E_HIP, "the passes counted %lld pairs, the compaction %lld", (long long)*n_pairs, (long long)cnt);
        HIP_TRY(nabo::agglom_sort_launch(*n_pairs, G.dhi.as<int64_t>(), G.dlo.as<uint64_t>(), G.sel[0].as<int32_t>(), G.sel[1].as<int32_t>(),
                                         G.key[0].as<uint64_t>(), G.key[1].as<uint64_t>(), H->temp.p, tb, nullptr));
    }
    if (T && (rc = T->stop(1))) return rc;
    return NABO_OK;
}

// comm of the current level from the first `take` pairs of the round
int agglom_set_comm(nabo_community *H, int64_t take)
{
    int rc = community_identity(H);
    if (rc) return rc;
    HIP_TRY(nabo::agglom_comm_launch(take, H->ag.sel[0].as<int32_t>(), H->ag.partner.as<int32_t>(), H->comm[H->cur].as<int32_t>(), nullptr));
    return NABO_OK;
}

int agglom_run(nabo_community *H, int64_t n_min)
{
    Agglom &G = H->ag;
    G.ran = false;
    G.merges.clear();
    G.q_path.clear();
    G.rounds = G.passes = G.peak = 0;
    for (double &m : G.ms) m = 0;
    int rc = agglom_reserve(H);
    if (rc) return rc;
    if ((rc = community_rewind(H))) return rc;
    nabo::PhaseTimer T{H->ev, G.ms, 3};
    G.rep_cur = 0;
    HIP_TRY(nabo::iota_launch(G.rep[0].as<uint32_t>(), H->n0, nullptr));
    std::vector<int64_t> rec;
    for (;;) {
        Level &lv = H->level();
        const int64_t n = lv.n;
        if (n <= n_min || lv.A == 0) break;
        int64_t n_pairs = 0, passes = 0;
        if ((rc = agglom_round(H, &n_pairs, &passes, &T))) return rc;
        G.passes += passes;
        if (n_pairs < 1) return nabo::api_fail(NABO_E_HIP, "a round on %lld arcs matched no pair", (long long)lv.A);
        const int64_t take = std::min(n_pairs, n - n_min);
        if ((rc = T.start())) return rc;
        HIP_TRY(nabo::agglom_records_launch(take, G.sel[0].as<int32_t>(), G.partner.as<int32_t>(), G.wa.as<int64_t>(), lv.k.as<int64_t>(),
                                            G.rep[G.rep_cur].as<int32_t>(), G.rounds, G.rec.as<int64_t>(), nullptr, nullptr));
        rec.resize((size_t)take * 6);
        HIP_TRY(hipMemcpy(rec.data(), G.rec.p, (size_t)take * 48, hipMemcpyDeviceToHost));
        G.merges.insert(G.merges.end(), rec.begin(), rec.end());
        if ((rc = T.stop(1))) return rc;
        if ((rc = T.start())) return rc;
        if ((rc = agglom_set_comm(H, take))) return rc;
        if ((rc = community_aggregate(H, nullptr, nullptr))) return rc;   // lv is gone; flag and newid hold the renumbering
        HIP_TRY(nabo::agglom_rep_launch(n, H->flag.as<int32_t>(), H->newid.as<int32_t>(), G.rep[G.rep_cur].as<int32_t>(),
                                        G.rep[G.rep_cur ^ 1].as<int32_t>(), nullptr));
        G.rep_cur ^= 1;
        if ((rc = T.stop(2))) return rc;
        ++G.rounds;
        if (H->level().n != n - take)
            return nabo::api_fail(NABO_E_HIP, "%lld merges left %lld of %lld clusters", (long long)take, (long long)H->level().n, (long long)n);
        if (take < n_pairs) break;
    }
    G.n_end = H->level().n;
    // the path of Q from the exact running sums, and its peak
    u128 si = 0, sd = 0;
    for (int64_t i = 0; i < H->n0; ++i) {
        si += (u128)H->h_in0[(size_t)i];
        sd += (u128)H->h_k0[(size_t)i] * (u128)H->h_k0[(size_t)i];
    }
    const size_t M = G.merges.size() / 6;
    G.q_path.resize(M + 1);
    __int128 best = (__int128)(si * (u128)H->two_m) - (__int128)sd;
    G.q_path[0] = modularity_of(si, sd, H->two_m, 1.0);
    for (size_t t = 1; t <= M; ++t) {
        const int64_t *r = &G.merges[6 * (t - 1)];
        si += 2 * (u128)r[3];
        sd += 2 * (u128)r[4] * (u128)r[5];
        G.q_path[t] = modularity_of(si, sd, H->two_m, 1.0);
        const __int128 x = (__int128)(si * (u128)H->two_m) - (__int128)sd;
        if (x > best) {
            best = x;
            G.peak = (int64_t)t;
        }
    }
    G.ran = true;
    return NABO_OK;
}

// the partition after the first t merges: parents from the merge list, pointer jumping, the numbering by size
int agglom_cut(nabo_community *H, int64_t t, std::vector<int32_t> &labels, int32_t *n_out)
{
    const int64_t n = H->n0;
    std::vector<int32_t> ra((size_t)t), rb((size_t)t);
    for (int64_t i = 0; i < t; ++i) {
        ra[(size_t)i] = (int32_t)H->ag.merges[(size_t)(6 * i)];
        rb[(size_t)i] = (int32_t)H->ag.merges[(size_t)(6 * i + 1)];
        if (ra[(size_t)i] < 0 || ra[(size_t)i] >= rb[(size_t)i] || rb[(size_t)i] >= n)
            return nabo::api_fail(NABO_E_HIP, "merge %lld joins %d and %d", (long long)i, (int)ra[(size_t)i], (int)rb[(size_t)i]);
    }
    HIP_TRY(nabo::iota_launch(H->lab.as<uint32_t>(), n, nullptr));
    if (t > 0) {   // flag, newid: the two columns of the prefix (t < n0)
        HIP_TRY(hipMemcpy(H->flag.p, ra.data(), (size_t)t * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(H->newid.p, rb.data(), (size_t)t * 4, hipMemcpyHostToDevice));
        HIP_TRY(nabo::agglom_parent_launch(t, H->flag.as<int32_t>(), H->newid.as<int32_t>(), H->lab.as<int32_t>(), nullptr));
        HIP_TRY(nabo::community_jump_launch(n, H->lab.as<int32_t>(), nullptr));
    }
    std::vector<int32_t> comp((size_t)n);
    HIP_TRY(hipMemcpy(comp.data(), H->lab.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return community_finish(H, comp.data(), 0, labels, n_out);
}

}  // namespace

extern "C" {

int nabo_community_geometry(int32_t *group, int32_t *long_threshold, int32_t *table_capacity)
{
    if (group) *group = nabo::CM_GROUP;
    if (long_threshold) *long_threshold = nabo::CM_LONG;
    if (table_capacity) *table_capacity = nabo::CM_CAP;
    return NABO_OK;
}

int nabo_community_create(nabo_community **out, int32_t device, int64_t n, const int64_t *ptr, const int64_t *nbr, const double *w,
                          double weight_scale)
{
    if (!out) return nabo::api_fail(NABO_E_INVALID, "out is NULL");
    *out = nullptr;
    if (n < 1) return nabo::api_fail(NABO_E_INVALID, "n=%lld must be at least 1", (long long)n);
    if (n >= ((int64_t)1 << 31)) return nabo::api_fail(NABO_E_UNSUPPORTED, "n=%lld: the clustering takes fewer than 2^31 nodes", (long long)n);
    if (!std::isfinite(weight_scale) || !(weight_scale > 0.0)) return nabo::api_fail(NABO_E_INVALID, "weight_scale must be finite and positive");
    int rc = nabo::check_csr_graph(n, ptr, nbr, w, nabo::CSR_FINITE_NOT_NEGATIVE);
    if (rc) return rc;
    if ((rc = nabo::use_device(device))) return rc;
    return nabo::create_handle(out, device, "nabo_community_create",
                               [&](nabo_community *H) { return community_create(H, n, ptr, nbr, w, weight_scale); });
}

void nabo_community_destroy(nabo_community *H)
{
    if (!H) return;
    (void)hipSetDevice(H->device);
    delete H;
}

int nabo_community_set_params(nabo_community *H, double resolution, uint64_t seed, int32_t max_sweeps, int32_t max_levels, int32_t split)
{
    if (!H) return nabo::api_fail(NABO_E_INVALID, "community is NULL");
    if (!std::isfinite(resolution) || resolution < 0.0) return nabo::api_fail(NABO_E_INVALID, "resolution must be finite and not negative");
    if (max_sweeps < 1 || max_levels < 1)
        return nabo::api_fail(NABO_E_INVALID, "max_sweeps=%d and max_levels=%d must be at least 1", (int)max_sweeps, (int)max_levels);
    H->gamma = resolution;
    H->seed = seed;
    H->max_sweeps = max_sweeps;
    H->max_levels = max_levels;
    H->split = split != 0;
    return NABO_OK;
}

int nabo_community_run(nabo_community *H)
{
    if (!H) return nabo::api_fail(NABO_E_INVALID, "community is NULL");
    int rc = nabo::use_device(H->device);
    if (rc) return rc;
    return community_run(H);
}

int nabo_community_labels(nabo_community *H, int32_t *labels, int32_t *n_clusters, double *q)
{
    if (!H) return nabo::api_fail(NABO_E_INVALID, "community is NULL");
    if (!H->ran) return nabo::api_fail(NABO_E_INVALID, "no run has finished on this handle");
    if (labels) memcpy(labels, H->labels.data(), (size_t)H->n0 * 4);
    if (n_clusters) *n_clusters = H->n_clusters;
    if (q) *q = H->q;
    return NABO_OK;
}

int nabo_community_history(nabo_community *H, int64_t *n_records, int64_t cap, int64_t *rec, double *q)
{
    if (!H) return nabo::api_fail(NABO_E_INVALID, "community is NULL");
    if (!H->ran) return nabo::api_fail(NABO_E_INVALID, "no run has finished on this handle");
    if (n_records) *n_records = (int64_t)H->history.size();
    for (int64_t r = 0; r < cap && r < (int64_t)H->history.size(); ++r) {
        const Record &R = H->history[(size_t)r];
        if (rec) {
            rec[4 * r] = R.n;
            rec[4 * r + 1] = R.n_next;
            rec[4 * r + 2] = R.sweeps;
            rec[4 * r + 3] = R.moved;
        }
        if (q) q[r] = R.q;
    }
    return NABO_OK;
}

int nabo_community_modularity(nabo_community *H, const int32_t *labels, double resolution, double *q)
{
    if (!H || !labels || !q) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    if (!std::isfinite(resolution)) return nabo::api_fail(NABO_E_INVALID, "resolution is not finite");
    int rc = nabo::use_device(H->device);
    if (rc) return rc;
    return community_modularity(H, labels, resolution, q);
}

int nabo_community_split(nabo_community *H, const int32_t *labels, int32_t split, int32_t *out, int32_t *n_clusters)
{
    if (!H || !labels || !out) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    int rc = nabo::use_device(H->device);
    if (rc) return rc;
    std::vector<int32_t> res;
    int32_t C = 0;
    rc = community_finish(H, labels, split != 0, res, &C);
    if (rc) return rc;
    memcpy(out, res.data(), (size_t)H->n0 * 4);
    if (n_clusters) *n_clusters = C;
    return NABO_OK;
}

int nabo_community_level_size(nabo_community *H, int64_t *n, int64_t *n_arcs, int64_t *two_m)
{
    if (!H) return nabo::api_fail(NABO_E_INVALID, "community is NULL");
    if (n) *n = H->level().n;
    if (n_arcs) *n_arcs = H->level().A;
    if (two_m) *two_m = H->two_m;
    return NABO_OK;
}

int nabo_community_get_level(nabo_community *H, int64_t *ptr, int64_t *nbr, int64_t *a, int64_t *k, int64_t *in)
{
    if (!H) return nabo::api_fail(NABO_E_INVALID, "community is NULL");
    int rc = nabo::use_device(H->device);
    if (rc) return rc;
    Level &lv = H->level();
    const size_t nb = (size_t)lv.n * 8, A = (size_t)lv.A;
    if (ptr) HIP_TRY(hipMemcpy(ptr, lv.ptr.p, nb + 8, hipMemcpyDeviceToHost));
    if (nbr && A) {
        std::vector<int32_t> h(A);
        HIP_TRY(hipMemcpy(h.data(), lv.nbr.p, A * 4, hipMemcpyDeviceToHost));
        for (size_t e = 0; e < A; ++e) nbr[e] = h[e];
    }
    if (a && A) HIP_TRY(hipMemcpy(a, lv.a.p, A * 8, hipMemcpyDeviceToHost));
    if (k) HIP_TRY(hipMemcpy(k, lv.k.p, nb, hipMemcpyDeviceToHost));
    if (in) HIP_TRY(hipMemcpy(in, lv.inn.p, nb, hipMemcpyDeviceToHost));
    return NABO_OK;
}

int nabo_community_set_comm(nabo_community *H, const int32_t *comm)
{
    if (!H || !comm) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    const int64_t n = H->level().n;
    for (int64_t i = 0; i < n; ++i)
        if (comm[i] < 0 || comm[i] >= n)
            return nabo::api_fail(NABO_E_INVALID, "comm[%lld] = %d is not a community in [0, %lld)", (long long)i, (int)comm[i], (long long)n);
    int rc = nabo::use_device(H->device);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(H->comm[H->cur].p, comm, (size_t)n * 4, hipMemcpyHostToDevice));
    return NABO_OK;
}

int nabo_community_get_comm(nabo_community *H, int32_t *comm)
{
    if (!H || !comm) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    int rc = nabo::use_device(H->device);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(comm, H->comm[H->cur].p, (size_t)H->level().n * 4, hipMemcpyDeviceToHost));
    return NABO_OK;
}

int nabo_community_sweep(nabo_community *H, int64_t level, int64_t sweep, int64_t *moved, int64_t *want)
{
    if (!H) return nabo::api_fail(NABO_E_INVALID, "community is NULL");
    if (level < 0 || sweep < 0) return nabo::api_fail(NABO_E_INVALID, "level=%lld or sweep=%lld is negative", (long long)level, (long long)sweep);
    int rc = nabo::use_device(H->device);
    if (rc) return rc;
    rc = H->counters.reserve(16);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(H->counters.p, 0, 16, nullptr));
    rc = community_sweep_enqueue(H, level, sweep, H->counters.as<uint64_t>());
    if (rc) return rc;
    uint64_t h[2];
    HIP_TRY(hipMemcpy(h, H->counters.p, 16, hipMemcpyDeviceToHost));
    if (moved) *moved = (int64_t)h[0];
    if (want) *want = (int64_t)h[1];
    return NABO_OK;
}

int nabo_community_aggregate(nabo_community *H)
{
    if (!H) return nabo::api_fail(NABO_E_INVALID, "community is NULL");
    int rc = nabo::use_device(H->device);
    if (rc) return rc;
    return community_aggregate(H, nullptr, nullptr);
}

int nabo_community_rewind(nabo_community *H)
{
    if (!H) return nabo::api_fail(NABO_E_INVALID, "community is NULL");
    int rc = nabo::use_device(H->device);
    if (rc) return rc;
    return community_rewind(H);
}

int nabo_community_last_ms(nabo_community *H, double ms[4])
{
    if (!H || !ms) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    for (int i = 0; i < 4; ++i) ms[i] = H->ms[i];
    return NABO_OK;
}

int nabo_community_agglomerate(nabo_community *H, int64_t n_min)
{
    if (!H) return nabo::api_fail(NABO_E_INVALID, "community is NULL");
    if (n_min < 1 || n_min > H->n0) return nabo::api_fail(NABO_E_INVALID, "n_min=%lld must be in [1, %lld]", (long long)n_min, (long long)H->n0);
    int rc = nabo::use_device(H->device);
    if (rc) return rc;
    return agglom_run(H, n_min);
}

int nabo_community_dendrogram(nabo_community *H, int64_t *n_merges, int64_t cap, int64_t *rec, double *q_path)
{
    if (!H) return nabo::api_fail(NABO_E_INVALID, "community is NULL");
    if (!H->ag.ran) return nabo::api_fail(NABO_E_INVALID, "no agglomeration has finished on this handle");
    const int64_t M = (int64_t)H->ag.merges.size() / 6, m = std::max<int64_t>(0, std::min(cap, M));
    if (n_merges) *n_merges = M;
    if (rec) memcpy(rec, H->ag.merges.data(), (size_t)m * 48);
    if (q_path) memcpy(q_path, H->ag.q_path.data(), (size_t)(m + 1) * 8);
    return NABO_OK;
}

int nabo_community_agglom_info(nabo_community *H, int64_t info[4])
{
    if (!H || !info) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    if (!H->ag.ran) return nabo::api_fail(NABO_E_INVALID, "no agglomeration has finished on this handle");
    info[0] = H->ag.rounds;
    info[1] = H->ag.passes;
    info[2] = H->ag.peak;
    info[3] = H->ag.n_end;
    return NABO_OK;
}

int nabo_community_cut(nabo_community *H, int64_t n_clusters, int32_t *labels, int32_t *n_out, double *q)
{
    if (!H) return nabo::api_fail(NABO_E_INVALID, "community is NULL");
    if (!H->ag.ran) return nabo::api_fail(NABO_E_INVALID, "no agglomeration has finished on this handle");
    const int64_t M = (int64_t)H->ag.merges.size() / 6;
    if (n_clusters != 0 && (n_clusters < H->n0 - M || n_clusters > H->n0))
        return nabo::api_fail(NABO_E_INVALID, "n_clusters=%lld is outside [%lld, %lld], the clusters at the end of the run and the nodes",
                              (long long)n_clusters, (long long)(H->n0 - M), (long long)H->n0);
    const int64_t t = n_clusters == 0 ? H->ag.peak : H->n0 - n_clusters;
    int rc = nabo::use_device(H->device);
    if (rc) return rc;
    std::vector<int32_t> res;
    int32_t C = 0;
    if ((rc = agglom_cut(H, t, res, &C))) return rc;
    if (C != H->n0 - t) return nabo::api_fail(NABO_E_HIP, "%lld merges left %d of %lld clusters", (long long)t, (int)C, (long long)H->n0);
    if (labels) memcpy(labels, res.data(), (size_t)H->n0 * 4);
    if (n_out) *n_out = C;
    if (q) *q = H->ag.q_path[(size_t)t];
    return NABO_OK;
}

int nabo_community_match_pass(nabo_community *H, const uint8_t *free, int32_t *partner, int64_t *d_hi, uint64_t *d_lo)
{
    if (!H) return nabo::api_fail(NABO_E_INVALID, "community is NULL");
    int rc = nabo::use_device(H->device);
    if (rc) return rc;
    if ((rc = agglom_reserve(H))) return rc;
    Agglom &G = H->ag;
    const size_t n = (size_t)H->level().n;
    if (free) {
        std::vector<uint8_t> f(n);
        for (size_t i = 0; i < n; ++i) f[i] = free[i] != 0;
        HIP_TRY(hipMemcpy(G.free.p, f.data(), n, hipMemcpyHostToDevice));
    } else
        HIP_TRY(hipMemset(G.free.p, 1, n));
    HIP_TRY(hipMemset(G.partner.p, 0xFF, n * 4));   // the pass leaves the rows that are not free alone: -1, D = 0
    HIP_TRY(hipMemset(G.dhi.p, 0, n * 8));
    HIP_TRY(hipMemset(G.dlo.p, 0, n * 8));
    if ((rc = agglom_pass_enqueue(H, false, G.partner.as<int32_t>(), G.dhi.as<int64_t>(), G.dlo.as<uint64_t>(), G.wa.as<int64_t>()))) return rc;
    if (partner) HIP_TRY(hipMemcpy(partner, G.partner.p, n * 4, hipMemcpyDeviceToHost));
    if (d_hi) HIP_TRY(hipMemcpy(d_hi, G.dhi.p, n * 8, hipMemcpyDeviceToHost));
    if (d_lo) HIP_TRY(hipMemcpy(d_lo, G.dlo.p, n * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipDeviceSynchronize());
    return NABO_OK;
}

int nabo_community_match(nabo_community *H, int64_t *n_pairs, int64_t *passes, int32_t *pairs)
{
    if (!H) return nabo::api_fail(NABO_E_INVALID, "community is NULL");
    int rc = nabo::use_device(H->device);
    if (rc) return rc;
    if ((rc = agglom_reserve(H))) return rc;
    int64_t m = 0, p = 0;
    if ((rc = agglom_round(H, &m, &p, nullptr))) return rc;
    if (pairs && m > 0) {
        HIP_TRY(nabo::agglom_records_launch(m, H->ag.sel[0].as<int32_t>(), H->ag.partner.as<int32_t>(), nullptr, nullptr, nullptr, 0, nullptr,
                                            H->ag.pairs.as<int32_t>(), nullptr));
        HIP_TRY(hipMemcpy(pairs, H->ag.pairs.p, (size_t)m * 8, hipMemcpyDeviceToHost));
    }
    if ((rc = agglom_set_comm(H, m))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    if (n_pairs) *n_pairs = m;
    if (passes) *passes = p;
    return NABO_OK;
}

int nabo_community_agglom_ms(nabo_community *H, double ms[4])
{
    if (!H || !ms) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    for (int i = 0; i < 4; ++i) ms[i] = H->ag.ms[i];
    return NABO_OK;
}

}  // extern "C"
