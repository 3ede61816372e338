// Unweighted hop distances on the reference SNN graph (nabo/_graph.py:794-824 get_mapping_specificity,
// :904-916 calc_contiguous_spl): for groups of reference nodes, the shortest-path length of every member pair.
//
// Resident graph.  The caller's CSR (rows in any arc direction, duplicates and self-loops allowed) becomes the
// undirected simple graph nx.Graph.add_edge would make: every arc is emitted in both directions as a 64-bit key
// (u << 32 | v), keys are radix-sorted (rocPRIM, stable), duplicates dropped, and int32 row pointers read off the
// sorted keys.  Self-loops stay: they change no distance.
//
// Two tiers answer a query; distances are integers, so both give the same bits and the split changes no output.
//   * local tier: one workgroup per group of <= 64 members, one bit per member POSITION.  A lockstep multi-source
//     BFS keeps, per reached node, OLD (bits of members within r-1 hops) and NEW (exactly r hops) in an LDS
//     open-addressing hash.  If members a and b first share a node at step r, D(a,b) is 2r-1 or 2r; it is 2r-1
//     exactly when some node is NEW for one of them and OLD for the other (a shortest path of odd length has a
//     node at r from one end and r-1 from the other; conversely such a node gives a path of 2r-1, and D < 2r-1
//     would have made them share at step r-1).  The search ends when every pair is resolved or the frontier
//     empties (the rest are unreachable).  A group whose table passes its capacity is handed on.
//   * global tier: level-synchronous multi-source BFS over the whole graph, 64 distinct sources per sweep, with
//     per-node uint64 visited / frontier masks updated by vector atomics.  A sweep carries the open pairs
//     (source slot, other node) of its sources; a pair resolves at the first level where the other node gains the
//     source's bit.  Sources are shared across groups: one BFS from s answers every pair of every group that
//     names s.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>
#include <stdint.h>

namespace nabo {

// ---- resident graph -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void paths_arcs_kernel(const int64_t *__restrict__ ptr, const int64_t *__restrict__ nbr,
                                                         int64_t n, uint64_t *__restrict__ keys)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    for (int64_t e = ptr[r]; e < ptr[r + 1]; ++e) {
        const uint64_t v = (uint64_t)nbr[e];
        keys[2 * e] = ((uint64_t)r << 32) | v;
        keys[2 * e + 1] = (v << 32) | (uint64_t)r;
    }
}

// rowptr[r] = first position of the sorted unique keys whose row is >= r; col = the low 32 bits
__global__ __launch_bounds__(256) void paths_rowptr_kernel(const uint64_t *__restrict__ keys, const int64_t *__restrict__ n_keys,
                                                           int64_t n, int32_t *__restrict__ rowptr, int32_t *__restrict__ col)
{
    const int64_t E = *n_keys;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i <= E; i += (int64_t)gridDim.x * 256) {
        const int64_t prev = i == 0 ? -1 : (int64_t)(keys[i - 1] >> 32);
        const int64_t cur = i == E ? n : (int64_t)(keys[i] >> 32);
        for (int64_t r = prev + 1; r <= cur; ++r) rowptr[r] = (int32_t)i;
        if (i < E) col[i] = (int32_t)(keys[i] & 0xFFFFFFFFull);
    }
}

static unsigned paths_key_bits(int64_t n)
{
    unsigned b = 1;
    while (b < 31 && ((int64_t)1 << b) < n) ++b;
    return 32 + b;
}

hipError_t paths_build_temp_bytes(int64_t E2, int64_t n, size_t *sort_bytes, size_t *uniq_bytes)
{
    *sort_bytes = *uniq_bytes = 0;
    hipError_t e = rocprim::radix_sort_keys(nullptr, *sort_bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)E2,
                                            0u, paths_key_bits(n), (hipStream_t) nullptr);
    if (e != hipSuccess) return e;
    return rocprim::unique(nullptr, *uniq_bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr, (int64_t *)nullptr,
                           (size_t)E2, rocprim::equal_to<uint64_t>(), (hipStream_t) nullptr);
}

// keys_a, keys_b: [2E] scratch; n_keys: one int64 on the device (number of distinct arcs, read back by the caller)
hipError_t paths_build_launch(const int64_t *ptr, const int64_t *nbr, int64_t n, int64_t E, uint64_t *keys_a, uint64_t *keys_b,
                              void *sort_temp, size_t sort_bytes, void *uniq_temp, size_t uniq_bytes, int64_t *n_keys,
                              int32_t *rowptr, int32_t *col, hipStream_t st)
{
    const int64_t E2 = 2 * E;
    hipError_t e = hipMemsetAsync(n_keys, 0, sizeof(int64_t), st);
    if (e != hipSuccess) return e;
    if (E > 0) {
        hipLaunchKernelGGL(paths_arcs_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ptr, nbr, n, keys_a);
        e = rocprim::radix_sort_keys(sort_temp, sort_bytes, (const uint64_t *)keys_a, keys_b, (size_t)E2, 0u, paths_key_bits(n), st);
        if (e != hipSuccess) return e;
        e = rocprim::unique(uniq_temp, uniq_bytes, (const uint64_t *)keys_b, keys_a, n_keys, (size_t)E2,
                            rocprim::equal_to<uint64_t>(), st);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(paths_rowptr_kernel, dim3(1024), dim3(256), 0, st, (const uint64_t *)keys_a, (const int64_t *)n_keys, n,
                       rowptr, col);
    return hipGetLastError();
}

// ---- local tier ---------------------------------------------------------------------------------------------------
// LDS layout (slots = power of two): keys[slots] i32 (-1 empty), old/cur/nxt[slots] u64, front[slots] i32.
constexpr int LOCAL_THREADS = 256;
constexpr int LOCAL_SUB = 16;          // lanes per frontier node while expanding (mean SNN degree ~16)

__device__ inline uint32_t paths_hash(int32_t v)
{
    const uint32_t h = (uint32_t)v * 2654435761u;
    return h ^ (h >> 15);
}

__global__ __launch_bounds__(LOCAL_THREADS) void paths_local_kernel(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const int64_t *__restrict__ grp_ptr,
    const int32_t *__restrict__ members, const int64_t *__restrict__ pair_off, const int32_t *__restrict__ groups,
    int32_t slots, int32_t limit, int32_t *__restrict__ pair_dist, int32_t *__restrict__ out_nodes)
{
    extern __shared__ uint64_t smem[];
    uint64_t *old_m = smem, *cur_m = smem + slots, *nxt_m = smem + 2 * slots;
    int32_t *keys = (int32_t *)(smem + 3 * slots), *front = keys + slots;
    __shared__ uint64_t share[64], odd[64], res[64];
    __shared__ int32_t n_front, n_nodes, n_front_next, overflow, open;

    const int tid = threadIdx.x;
    const int32_t g = groups[blockIdx.x];
    const int64_t m0 = grp_ptr[g];
    const int m = (int)(grp_ptr[g + 1] - m0);
    const int64_t poff = pair_off[g];
    const uint32_t mask = (uint32_t)slots - 1;

    for (int i = tid; i < slots; i += LOCAL_THREADS) {
        keys[i] = -1;
        old_m[i] = 0;
        cur_m[i] = 0;
        nxt_m[i] = 0;
    }
    if (tid < 64) { share[tid] = 0; odd[tid] = 0; res[tid] = 0; }
    if (tid == 0) { n_front = 0; n_nodes = 0; n_front_next = 0; overflow = 0; }
    __syncthreads();

    // insert v (or find it); returns its slot, -1 when the table is past its capacity
    auto insert = [&](int32_t v) -> int {
        uint32_t h = paths_hash(v) & mask;
        for (int probe = 0; probe < slots; ++probe, h = (h + 1) & mask) {
            const int32_t k = keys[h];
            if (k == v) return (int)h;
            if (k == -1) {
                const int32_t was = atomicCAS(&keys[h], -1, v);
                if (was == -1) {
                    if (atomicAdd(&n_nodes, 1) >= limit) { atomicOr(&overflow, 1); return -1; }
                    return (int)h;
                }
                if (was == v) return (int)h;
            }
        }
        atomicOr(&overflow, 1);
        return -1;
    };

    // step 0: every member position sets its bit on its node (repeated members share a node)
    if (tid < m) {
        const int s = insert(members[m0 + tid]);
        if (s >= 0) atomicOr((unsigned long long *)&nxt_m[s], 1ull << tid);
    }
    __syncthreads();
    const uint64_t all = m == 64 ? ~0ull : ((1ull << m) - 1);
    for (int r = 0; !overflow; ++r) {
        // fold: NEW = what arrived this step minus what was there; OLD |= previous NEW; collect the frontier
        for (int i = tid; i < slots; i += LOCAL_THREADS) {
            if (keys[i] == -1) continue;
            const uint64_t o = old_m[i] | cur_m[i];
            const uint64_t nw = nxt_m[i] & ~o;
            old_m[i] = o;
            cur_m[i] = nw;
            nxt_m[i] = 0;
            if (nw) {
                front[atomicAdd(&n_front_next, 1)] = i;
                // pairs that meet here: (new, new) and (new, old) -- the latter witness an odd distance
                for (uint64_t b = nw; b; b &= b - 1) {
                    const int a = __ffsll((unsigned long long)b) - 1;
                    atomicOr((unsigned long long *)&share[a], o | nw);
                    if (o) atomicOr((unsigned long long *)&odd[a], o);
                }
                for (uint64_t b = o; b; b &= b - 1) {
                    const int a = __ffsll((unsigned long long)b) - 1;
                    atomicOr((unsigned long long *)&share[a], nw);
                    atomicOr((unsigned long long *)&odd[a], nw);
                }
            }
        }
        if (tid == 0) open = 0;
        __syncthreads();
        if (tid < m) {
            const uint64_t later = all & ~((2ull << tid) - 1);     // positions j > tid
            const uint64_t newly = share[tid] & later & ~res[tid];
            for (uint64_t b = newly; b; b &= b - 1) {
                const int j = __ffsll((unsigned long long)b) - 1;
                const int64_t idx = (int64_t)tid * m - (int64_t)tid * (tid + 1) / 2 + (j - tid - 1);
                pair_dist[poff + idx] = ((odd[tid] >> j) & 1) && r > 0 ? 2 * r - 1 : 2 * r;
            }
            res[tid] |= newly;
            if (later & ~res[tid]) atomicOr(&open, 1);
        }
        if (tid == 0) { n_front = n_front_next; n_front_next = 0; }
        __syncthreads();
        if (!open) break;
        if (n_front == 0) {
            // the balls stopped growing: every pair still open is unreachable
            if (tid < m) {
                const uint64_t left = all & ~((2ull << tid) - 1) & ~res[tid];
                for (uint64_t b = left; b; b &= b - 1) {
                    const int j = __ffsll((unsigned long long)b) - 1;
                    pair_dist[poff + (int64_t)tid * m - (int64_t)tid * (tid + 1) / 2 + (j - tid - 1)] = -1;
                }
            }
            break;
        }
        // expand: LOCAL_SUB lanes per frontier node
        const int sub = tid / LOCAL_SUB, lane = tid % LOCAL_SUB;
        for (int f = sub; f < n_front; f += LOCAL_THREADS / LOCAL_SUB) {
            const int s = front[f];
            const int32_t u = keys[s];
            const uint64_t bits = cur_m[s];
            for (int32_t e = rowptr[u] + lane; e < rowptr[u + 1]; e += LOCAL_SUB) {
                const int t = insert(col[e]);
                if (t < 0) break;
                atomicOr((unsigned long long *)&nxt_m[t], bits);
            }
        }
        __syncthreads();
    }
    if (tid == 0) out_nodes[blockIdx.x] = overflow ? -1 : (n_nodes < limit ? n_nodes : limit);
}

hipError_t paths_local_launch(const int32_t *rowptr, const int32_t *col, const int64_t *grp_ptr, const int32_t *members,
                              const int64_t *pair_off, const int32_t *groups, int64_t n_local, int32_t slots, int32_t limit,
                              int32_t *pair_dist, int32_t *out_nodes, hipStream_t st)
{
    if (n_local == 0) return hipSuccess;
    const size_t lds = (size_t)slots * (3 * sizeof(uint64_t) + 2 * sizeof(int32_t));
    hipLaunchKernelGGL(paths_local_kernel, dim3((unsigned)n_local), dim3(LOCAL_THREADS), lds, st, rowptr, col, grp_ptr, members,
                       pair_off, groups, slots, limit, pair_dist, out_nodes);
    return hipGetLastError();
}

// ---- global tier --------------------------------------------------------------------------------------------------
struct PathsPair {
    int32_t t;          // the other node
    int32_t slot;       // source bit in the sweep; -1: both ends are the same node (distance 0)
    int64_t out;        // position in pair_dist
};

// counters: [0] next-frontier length, [1] pairs resolved this level, [2] touched length, [3] current-frontier length
__global__ __launch_bounds__(256) void paths_prefill_kernel(const PathsPair *__restrict__ pairs, int64_t n,
                                                            int32_t *__restrict__ pair_dist)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) pair_dist[pairs[i].out] = pairs[i].slot < 0 ? 0 : -1;
}

__global__ __launch_bounds__(64) void paths_sweep_init_kernel(const int32_t *__restrict__ src, int n_src, uint64_t *__restrict__ visited,
                                                              uint64_t *__restrict__ front, int32_t *__restrict__ cur,
                                                              int32_t *__restrict__ touched, int64_t *__restrict__ counters)
{
    const int s = threadIdx.x;
    if (s < n_src) {
        const int32_t v = src[s];
        visited[v] = 1ull << s;
        front[v] = 1ull << s;
        cur[s] = v;
        touched[s] = v;
    }
    if (s == 0) {
        counters[0] = 0;
        counters[1] = 0;
        counters[2] = n_src;
        counters[3] = n_src;
    }
}

constexpr int GLOBAL_SUB = 16;

__global__ __launch_bounds__(256) void paths_expand_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                           const int32_t *__restrict__ cur, const uint64_t *__restrict__ visited,
                                                           const uint64_t *__restrict__ front, uint64_t *__restrict__ nxt,
                                                           int32_t *__restrict__ next_list, int64_t *__restrict__ counters)
{
    const int64_t n_cur = counters[3];
    const int lane = threadIdx.x % GLOBAL_SUB;
    for (int64_t f = ((int64_t)blockIdx.x * 256 + threadIdx.x) / GLOBAL_SUB; f < n_cur; f += (int64_t)gridDim.x * (256 / GLOBAL_SUB)) {
        const int32_t u = cur[f];
        const uint64_t bits = front[u];
        for (int32_t e = rowptr[u] + lane; e < rowptr[u + 1]; e += GLOBAL_SUB) {
            const int32_t v = col[e];
            const uint64_t add = bits & ~visited[v];
            if (!add) continue;
            const uint64_t was = atomicOr((unsigned long long *)&nxt[v], (unsigned long long)add);
            if (was == 0) next_list[atomicAdd((unsigned long long *)&counters[0], 1ull)] = v;
        }
    }
}

// pairs whose other end gained the source bit at this level resolve; the old frontier's masks are cleared
__global__ __launch_bounds__(256) void paths_check_kernel(const PathsPair *__restrict__ pairs, int64_t n_pairs, int32_t level,
                                                          const uint64_t *__restrict__ nxt, const int32_t *__restrict__ cur,
                                                          uint64_t *__restrict__ front, int32_t *__restrict__ pair_dist,
                                                          int64_t *__restrict__ counters)
{
    const int64_t n_cur = counters[3];
    const int64_t stride = (int64_t)gridDim.x * 256;
    int resolved = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_pairs; i += stride) {
        const PathsPair p = pairs[i];
        if (pair_dist[p.out] == -1 && ((nxt[p.t] >> p.slot) & 1)) {
            pair_dist[p.out] = level;
            ++resolved;
        }
    }
    if (resolved) atomicAdd((unsigned long long *)&counters[1], (unsigned long long)resolved);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_cur; i += stride) front[cur[i]] = 0;
}

__global__ __launch_bounds__(256) void paths_finalize_kernel(const int32_t *__restrict__ next_list, uint64_t *__restrict__ visited,
                                                             uint64_t *__restrict__ front, uint64_t *__restrict__ nxt,
                                                             int32_t *__restrict__ touched, int64_t *__restrict__ counters)
{
    const int64_t n_next = counters[0];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_next; i += (int64_t)gridDim.x * 256) {
        const int32_t v = next_list[i];
        const uint64_t b = nxt[v], was = visited[v];
        visited[v] = was | b;
        front[v] = b;
        nxt[v] = 0;
        if (was == 0) touched[atomicAdd((unsigned long long *)&counters[2], 1ull)] = v;
    }
}

// next frontier becomes the current one (the caller swaps the list pointers)
__global__ void paths_advance_kernel(int64_t *__restrict__ counters)
{
    if (threadIdx.x == 0) {
        counters[3] = counters[0];
        counters[0] = 0;
        counters[1] = 0;
    }
}

__global__ __launch_bounds__(256) void paths_clear_kernel(const int32_t *__restrict__ touched, const int64_t *__restrict__ counters,
                                                          uint64_t *__restrict__ visited, uint64_t *__restrict__ front)
{
    const int64_t n = counters[2];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        visited[touched[i]] = 0;
        front[touched[i]] = 0;
    }
}

// ---- levels around node sets (nabo_refgraph_set_levels): the same sweep with one bit per SET -------------------------
// seeds: member i of the sweep sets bit seed_bit[i] on node seed_node[i].  A node may sit in several sets and a set
// may name a node twice, so the masks are OR-ed; the thread that finds the node untouched lists it (once) in the
// frontier and in the touched list.  counters must be zero before the launch.
__global__ __launch_bounds__(256) void paths_seed_sets_kernel(const int32_t *__restrict__ seed_node, const uint8_t *__restrict__ seed_bit,
                                                              int64_t n_seeds, int64_t n, uint64_t *__restrict__ visited,
                                                              uint64_t *__restrict__ front, int32_t *__restrict__ cur,
                                                              int32_t *__restrict__ touched, int64_t *__restrict__ counters,
                                                              int32_t *__restrict__ level)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_seeds; i += (int64_t)gridDim.x * 256) {
        const int32_t v = seed_node[i];
        const int s = seed_bit[i];
        const uint64_t was = atomicOr((unsigned long long *)&visited[v], 1ull << s);
        atomicOr((unsigned long long *)&front[v], 1ull << s);
        level[(int64_t)s * n + v] = 0;
        if (was == 0) {
            cur[atomicAdd((unsigned long long *)&counters[3], 1ull)] = v;
            touched[atomicAdd((unsigned long long *)&counters[2], 1ull)] = v;
        }
    }
}

// after an expansion nxt[v] holds exactly the bits v gains at this level (expand masks out what v had): record them,
// and clear the old frontier's masks as paths_check_kernel does
__global__ __launch_bounds__(256) void paths_record_kernel(const int32_t *__restrict__ next_list, const uint64_t *__restrict__ nxt,
                                                           const int32_t *__restrict__ cur, uint64_t *__restrict__ front, int64_t n,
                                                           int32_t lvl, int32_t *__restrict__ level, const int64_t *__restrict__ counters)
{
    const int64_t n_next = counters[0], n_cur = counters[3];
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_next; i += stride) {
        const int32_t v = next_list[i];
        for (uint64_t b = nxt[v]; b; b &= b - 1) level[(int64_t)(__ffsll((unsigned long long)b) - 1) * n + v] = lvl;
    }
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_cur; i += stride) front[cur[i]] = 0;
}

hipError_t paths_seed_sets_launch(const int32_t *seed_node, const uint8_t *seed_bit, int64_t n_seeds, int64_t n, uint64_t *visited,
                                  uint64_t *front, int32_t *cur, int32_t *touched, int64_t *counters, int32_t *level, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(counters, 0, 4 * sizeof(int64_t), st);
    if (e != hipSuccess || n_seeds == 0) return e;
    const int64_t want = (n_seeds + 255) / 256;
    hipLaunchKernelGGL(paths_seed_sets_kernel, dim3((unsigned)(want > 1024 ? 1024 : want)), dim3(256), 0, st, seed_node, seed_bit, n_seeds,
                       n, visited, front, cur, touched, counters, level);
    return hipGetLastError();
}

// one level of a set sweep: expand, record the levels gained, fold the next frontier in
hipError_t paths_set_level_launch(const int32_t *rowptr, const int32_t *col, const int32_t *cur, int32_t *next_list, uint64_t *visited,
                                  uint64_t *front, uint64_t *nxt, int32_t *touched, int64_t n, int32_t lvl, int32_t *level,
                                  int64_t *counters, int64_t n_cur_hint, hipStream_t st)
{
    const int64_t want = (n_cur_hint * GLOBAL_SUB + 255) / 256;
    const unsigned g_exp = (unsigned)(want < 1 ? 1 : want > 4096 ? 4096 : want);
    hipLaunchKernelGGL(paths_expand_kernel, dim3(g_exp), dim3(256), 0, st, rowptr, col, cur, (const uint64_t *)visited,
                       (const uint64_t *)front, nxt, next_list, counters);
    hipLaunchKernelGGL(paths_record_kernel, dim3(1024), dim3(256), 0, st, (const int32_t *)next_list, (const uint64_t *)nxt, cur, front, n,
                       lvl, level, (const int64_t *)counters);
    hipLaunchKernelGGL(paths_finalize_kernel, dim3(1024), dim3(256), 0, st, (const int32_t *)next_list, visited, front, nxt, touched,
                       counters);
    return hipGetLastError();
}

hipError_t paths_prefill_launch(const void *pairs, int64_t n, int32_t *pair_dist, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(paths_prefill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const PathsPair *)pairs, n, pair_dist);
    return hipGetLastError();
}

hipError_t paths_sweep_init_launch(const int32_t *src, int n_src, uint64_t *visited, uint64_t *front, int32_t *cur,
                                   int32_t *touched, int64_t *counters, hipStream_t st)
{
    hipLaunchKernelGGL(paths_sweep_init_kernel, dim3(1), dim3(64), 0, st, src, n_src, visited, front, cur, touched, counters);
    return hipGetLastError();
}

// one level: expand the current frontier, resolve pairs, fold the next frontier in; the caller reads counters[0..1]
hipError_t paths_level_launch(const int32_t *rowptr, const int32_t *col, const int32_t *cur, int32_t *next_list, uint64_t *visited,
                              uint64_t *front, uint64_t *nxt, int32_t *touched, const void *pairs, int64_t n_pairs, int32_t level,
                              int32_t *pair_dist, int64_t *counters, int64_t n_cur_hint, hipStream_t st)
{
    const int64_t want = (n_cur_hint * GLOBAL_SUB + 255) / 256;
    const unsigned g_exp = (unsigned)(want < 1 ? 1 : want > 4096 ? 4096 : want);
    hipLaunchKernelGGL(paths_expand_kernel, dim3(g_exp), dim3(256), 0, st, rowptr, col, cur, (const uint64_t *)visited,
                       (const uint64_t *)front, nxt, next_list, counters);
    const int64_t wc = ((n_pairs > n_cur_hint ? n_pairs : n_cur_hint) + 255) / 256;
    const unsigned g_chk = (unsigned)(wc < 1 ? 1 : wc > 4096 ? 4096 : wc);
    hipLaunchKernelGGL(paths_check_kernel, dim3(g_chk), dim3(256), 0, st, (const PathsPair *)pairs, n_pairs, level,
                       (const uint64_t *)nxt, cur, front, pair_dist, counters);
    hipLaunchKernelGGL(paths_finalize_kernel, dim3(1024), dim3(256), 0, st, (const int32_t *)next_list, visited, front, nxt, touched,
                       counters);
    return hipGetLastError();
}

hipError_t paths_advance_launch(int64_t *counters, hipStream_t st)
{
    hipLaunchKernelGGL(paths_advance_kernel, dim3(1), dim3(64), 0, st, counters);
    return hipGetLastError();
}

hipError_t paths_clear_launch(const int32_t *touched, const int64_t *counters, uint64_t *visited, uint64_t *front, hipStream_t st)
{
    hipLaunchKernelGGL(paths_clear_kernel, dim3(1024), dim3(256), 0, st, touched, counters, visited, front);
    return hipGetLastError();
}

// ---- per-group totals ---------------------------------------------------------------------------------------------
// one wavefront per group: sum of the pair distances >= 0 and the number of unreachable (-1) pairs
__global__ __launch_bounds__(256) void paths_reduce_kernel(const int64_t *__restrict__ pair_off, int64_t n_groups,
                                                           const int32_t *__restrict__ pair_dist, int64_t *__restrict__ out_sum,
                                                           int64_t *__restrict__ out_unreached)
{
    const int64_t g = (int64_t)blockIdx.x * 4 + threadIdx.x / 64;
    const int lane = threadIdx.x % 64;
    if (g >= n_groups) return;
    long long s = 0, u = 0;
    for (int64_t i = pair_off[g] + lane; i < pair_off[g + 1]; i += 64) {
        const int32_t d = pair_dist[i];
        if (d < 0) ++u;
        else s += d;
    }
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o, 64);
        u += __shfl_xor(u, o, 64);
    }
    if (lane == 0) {
        out_sum[g] = s;
        out_unreached[g] = u;
    }
}

hipError_t paths_reduce_launch(const int64_t *pair_off, int64_t n_groups, const int32_t *pair_dist, int64_t *out_sum,
                               int64_t *out_unreached, hipStream_t st)
{
    if (n_groups == 0) return hipSuccess;
    hipLaunchKernelGGL(paths_reduce_kernel, dim3((unsigned)((n_groups + 3) / 4)), dim3(256), 0, st, pair_off, n_groups, pair_dist,
                       out_sum, out_unreached);
    return hipGetLastError();
}

}  // namespace nabo

// ---- C ABI (include/nabo_graph.h) ---------------------------------------------------------------------------------
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/nabo_cluster.h"
#include "../../include/nabo_graph.h"
#include "../../include/nabo_knn.h"
#include "host_common.h"

namespace {

using nabo::DevBuf;
using nabo::PathsPair;
using nabo::use_device;

constexpr int64_t LOCAL_CAPACITY_MAX = 896;     // 1024 slots x 32 B of LDS
// measured balls (DESIGN.md "Hop distances"): the nodes within ceil(Dmax/2) of a group's members are <= 115 for 90 %
// of c1_3k's targets and <= 380 for 99 % of mapping_small's; 768 holds both with the table <= 3/4 full
constexpr int64_t LOCAL_CAPACITY_DEFAULT = 768;

double now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

}  // namespace

struct nabo_refgraph {
    int device = 0;
    int64_t n = 0, n_arcs = 0;
    hipStream_t st = nullptr;
    DevBuf rowptr, col;
    // global-tier state, allocated on first use: visited / frontier / next masks, node lists, counters
    DevBuf visited, front, nxt, cur, next_list, touched, counters;
    int64_t *host_counters = nullptr;     // pinned
    int64_t local_capacity = LOCAL_CAPACITY_DEFAULT, local_max_members = 64;
    double build_ms = 0;
    double ms[4] = {0, 0, 0, 0};
    int64_t stats[4] = {0, 0, 0, 0};
    std::vector<int32_t> local_nodes;
    ~nabo_refgraph()
    {
        if (host_counters) (void)hipHostFree(host_counters);
        if (st) (void)hipStreamDestroy(st);
    }
};

namespace {

int refgraph_build(nabo_refgraph *g, const int64_t *ptr, const int64_t *nbr)
{
    const int64_t n = g->n, E = ptr[n];
    size_t sort_bytes = 0, uniq_bytes = 0;
    HIP_TRY(nabo::paths_build_temp_bytes(2 * E, n, &sort_bytes, &uniq_bytes));
    DevBuf d_ptr, d_nbr, keys_a, keys_b, sort_temp, uniq_temp, n_keys;
    HIP_TRY(d_ptr.alloc((size_t)(n + 1) * 8));
    HIP_TRY(d_nbr.alloc((size_t)E * 8));
    HIP_TRY(keys_a.alloc((size_t)2 * E * 8));
    HIP_TRY(keys_b.alloc((size_t)2 * E * 8));
    HIP_TRY(sort_temp.alloc(sort_bytes));
    HIP_TRY(uniq_temp.alloc(uniq_bytes));
    HIP_TRY(n_keys.alloc(8));
    HIP_TRY(hipMemcpyAsync(d_ptr.p, ptr, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, g->st));
    if (E) HIP_TRY(hipMemcpyAsync(d_nbr.p, nbr, (size_t)E * 8, hipMemcpyHostToDevice, g->st));
    HIP_TRY(g->rowptr.alloc((size_t)(n + 1) * 4));
    HIP_TRY(g->col.alloc((size_t)2 * E * 4));
    HIP_TRY(nabo::paths_build_launch(d_ptr.as<int64_t>(), d_nbr.as<int64_t>(), n, E, keys_a.as<uint64_t>(), keys_b.as<uint64_t>(),
                                     sort_temp.p, sort_bytes, uniq_temp.p, uniq_bytes, n_keys.as<int64_t>(),
                                     g->rowptr.as<int32_t>(), g->col.as<int32_t>(), g->st));
    int64_t arcs = 0;
    HIP_TRY(hipMemcpyAsync(&arcs, n_keys.p, 8, hipMemcpyDeviceToHost, g->st));
    HIP_TRY(hipStreamSynchronize(g->st));
    g->n_arcs = arcs;
    return NABO_OK;
}

int ensure_global_state(nabo_refgraph *g)
{
    if (g->visited.p) return NABO_OK;
    const size_t n = (size_t)g->n;
    HIP_TRY(g->visited.alloc(n * 8));
    HIP_TRY(g->front.alloc(n * 8));
    HIP_TRY(g->nxt.alloc(n * 8));
    HIP_TRY(g->cur.alloc(n * 4));
    HIP_TRY(g->next_list.alloc(n * 4));
    HIP_TRY(g->touched.alloc(n * 4));
    HIP_TRY(g->counters.alloc(4 * 8));
    HIP_TRY(hipHostMalloc((void **)&g->host_counters, 4 * 8, hipHostMallocDefault));
    HIP_TRY(hipMemsetAsync(g->visited.p, 0, n * 8, g->st));
    HIP_TRY(hipMemsetAsync(g->front.p, 0, n * 8, g->st));
    HIP_TRY(hipMemsetAsync(g->nxt.p, 0, n * 8, g->st));
    return NABO_OK;
}

// sweeps of <= 64 sources over the open pairs, sorted by sweep (pairs [sweep_ptr[w], sweep_ptr[w+1]))
int run_global(nabo_refgraph *g, const std::vector<int32_t> &sources, const std::vector<int64_t> &sweep_ptr,
               const PathsPair *d_pairs, int32_t *d_pair_dist)
{
    int rc = ensure_global_state(g);
    if (rc) return rc;
    DevBuf d_src;
    HIP_TRY(d_src.alloc(sources.size() * 4));
    if (!sources.empty())
        HIP_TRY(hipMemcpyAsync(d_src.p, sources.data(), sources.size() * 4, hipMemcpyHostToDevice, g->st));
    int32_t *cur = g->cur.as<int32_t>(), *nxt_list = g->next_list.as<int32_t>();
    int64_t *cnt = g->counters.as<int64_t>();
    const int64_t n_sweeps = (int64_t)sweep_ptr.size() - 1;
    for (int64_t w = 0; w < n_sweeps; ++w) {
        const int n_src = (int)std::min<int64_t>(64, (int64_t)sources.size() - 64 * w);
        const int64_t p0 = sweep_ptr[w], np = sweep_ptr[w + 1] - p0;
        HIP_TRY(nabo::paths_sweep_init_launch(d_src.as<int32_t>() + 64 * w, n_src, g->visited.as<uint64_t>(), g->front.as<uint64_t>(),
                                              cur, g->touched.as<int32_t>(), cnt, g->st));
        int64_t open = np, n_cur = n_src;
        int32_t level = 0;
        while (open > 0 && n_cur > 0) {
            ++level;
            HIP_TRY(nabo::paths_level_launch(g->rowptr.as<int32_t>(), g->col.as<int32_t>(), cur, nxt_list, g->visited.as<uint64_t>(),
                                             g->front.as<uint64_t>(), g->nxt.as<uint64_t>(), g->touched.as<int32_t>(), d_pairs + p0,
                                             np, level, d_pair_dist, cnt, n_cur, g->st));
            HIP_TRY(hipMemcpyAsync(g->host_counters, cnt, 2 * 8, hipMemcpyDeviceToHost, g->st));
            HIP_TRY(nabo::paths_advance_launch(cnt, g->st));
            HIP_TRY(hipStreamSynchronize(g->st));
            n_cur = g->host_counters[0];
            open -= g->host_counters[1];
            std::swap(cur, nxt_list);
        }
        g->stats[3] = std::max<int64_t>(g->stats[3], level);
        HIP_TRY(nabo::paths_clear_launch(g->touched.as<int32_t>(), cnt, g->visited.as<uint64_t>(), g->front.as<uint64_t>(), g->st));
    }
    // the lists may have been swapped an odd number of times: keep the object's pointers as they are (both are scratch)
    HIP_TRY(hipStreamSynchronize(g->st));
    g->stats[2] += n_sweeps;
    return NABO_OK;
}

inline int64_t n_pairs_of(int64_t m) { return m < 2 ? 0 : m * (m - 1) / 2; }

}  // namespace

extern "C" {

int nabo_refgraph_create(nabo_refgraph **out, int32_t device, int64_t n_nodes, const int64_t *ptr, const int64_t *nbr)
{
    if (!out) return nabo::api_fail(NABO_E_INVALID, "out is NULL");
    *out = nullptr;
    if (n_nodes < 0 || n_nodes >= ((int64_t)1 << 31) - 1) return nabo::api_fail(NABO_E_INVALID, "n_nodes=%lld out of range [0, 2^31 - 1)", (long long)n_nodes);
    int rc = nabo::check_csr_ptr("ptr", "row", n_nodes, ptr);
    if (rc) return rc;
    const int64_t E = ptr[n_nodes];
    if (E >= ((int64_t)1 << 30)) return nabo::api_fail(NABO_E_UNSUPPORTED, "%lld arcs: fewer than 2^30 per graph", (long long)E);
    if (E > 0 && !nbr) return nabo::api_fail(NABO_E_INVALID, "nbr is NULL");
    for (int64_t e = 0; e < E; ++e)
        if (nbr[e] < 0 || nbr[e] >= n_nodes)
            return nabo::api_fail(NABO_E_INVALID, "nbr[%lld] = %lld is not a node index in [0, %lld)", (long long)e, (long long)nbr[e], (long long)n_nodes);
    if ((rc = use_device(device))) return rc;
    nabo_refgraph *g = new (std::nothrow) nabo_refgraph();
    if (!g) return nabo::api_fail(NABO_E_NOMEM, "host allocation failed");
    g->device = device;
    g->n = n_nodes;
    const double t0 = now_ms();
    hipError_t e = hipStreamCreateWithFlags(&g->st, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete g;
        return nabo::api_fail(NABO_E_HIP, "stream creation failed: %s", hipGetErrorString(e));
    }
    rc = refgraph_build(g, ptr, nbr);
    if (rc) {
        delete g;
        return rc;
    }
    g->build_ms = now_ms() - t0;
    g->ms[0] = g->build_ms;
    *out = g;
    return NABO_OK;
}

int nabo_refgraph_destroy(nabo_refgraph *g)
{
    if (!g) return NABO_OK;
    (void)hipSetDevice(g->device);
    (void)hipStreamSynchronize(g->st);
    delete g;
    return NABO_OK;
}

int nabo_refgraph_set_option(nabo_refgraph *g, const char *name, int64_t value)
{
    if (!g || !name) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    if (!strcmp(name, "local_capacity")) {
        if (value < 0 || value > LOCAL_CAPACITY_MAX)
            return nabo::api_fail(NABO_E_INVALID, "local_capacity=%lld outside [0, %lld]", (long long)value, (long long)LOCAL_CAPACITY_MAX);
        g->local_capacity = value;
    } else if (!strcmp(name, "local_max_members")) {
        if (value < 2 || value > 64) return nabo::api_fail(NABO_E_INVALID, "local_max_members=%lld outside [2, 64]", (long long)value);
        g->local_max_members = value;
    } else {
        return nabo::api_fail(NABO_E_INVALID, "unknown option '%s'", name);
    }
    return NABO_OK;
}

int nabo_refgraph_group_hops(nabo_refgraph *g, int64_t n_groups, const int64_t *grp_ptr, const int64_t *members,
                             int64_t *out_sum, int64_t *out_unreached, int32_t *out_pair_hops)
{
    if (!g) return nabo::api_fail(NABO_E_INVALID, "NULL graph");
    if (n_groups < 0 || n_groups >= ((int64_t)1 << 31)) return nabo::api_fail(NABO_E_INVALID, "n_groups=%lld out of range", (long long)n_groups);
    if (!grp_ptr || (n_groups > 0 && (!out_sum || !out_unreached))) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    if (grp_ptr[0] != 0) return nabo::api_fail(NABO_E_INVALID, "grp_ptr[0] = %lld, must be 0", (long long)grp_ptr[0]);
    std::vector<int64_t> pair_off((size_t)n_groups + 1, 0);
    for (int64_t i = 0; i < n_groups; ++i) {
        const int64_t m = grp_ptr[i + 1] - grp_ptr[i];
        if (m < 0) return nabo::api_fail(NABO_E_INVALID, "grp_ptr is not monotone at group %lld", (long long)i);
        if (m > ((int64_t)1 << 20)) return nabo::api_fail(NABO_E_UNSUPPORTED, "group %lld has %lld members (at most 2^20)", (long long)i, (long long)m);
        pair_off[i + 1] = pair_off[i] + n_pairs_of(m);
    }
    const int64_t M = grp_ptr[n_groups], P = pair_off[n_groups];
    if (M > 0 && !members) return nabo::api_fail(NABO_E_INVALID, "members is NULL");
    if (M >= ((int64_t)1 << 31)) return nabo::api_fail(NABO_E_UNSUPPORTED, "%lld members: fewer than 2^31 per call", (long long)M);
    std::vector<int32_t> mem((size_t)M);
    for (int64_t i = 0; i < M; ++i) {
        if (members[i] < 0 || members[i] >= g->n)
            return nabo::api_fail(NABO_E_INVALID, "members[%lld] = %lld is not a node index in [0, %lld)", (long long)i, (long long)members[i], (long long)g->n);
        mem[i] = (int32_t)members[i];
    }
    int rc = use_device(g->device);
    if (rc) return rc;
    const double t0 = now_ms();
    for (int i = 1; i < 4; ++i) g->ms[i] = 0;
    for (int i = 0; i < 4; ++i) g->stats[i] = 0;
    g->ms[0] = g->build_ms;

    std::vector<int32_t> local;
    const bool use_local = g->local_capacity > 0;
    for (int64_t i = 0; i < n_groups; ++i) {
        const int64_t m = grp_ptr[i + 1] - grp_ptr[i];
        if (use_local && m >= 2 && m <= g->local_max_members) local.push_back((int32_t)i);
    }
    DevBuf d_grp, d_mem, d_off, d_local, d_dist, d_nodes, d_sum, d_unr;
    HIP_TRY(d_grp.alloc((size_t)(n_groups + 1) * 8));
    HIP_TRY(d_mem.alloc((size_t)M * 4));
    HIP_TRY(d_off.alloc((size_t)(n_groups + 1) * 8));
    HIP_TRY(d_local.alloc(local.size() * 4));
    HIP_TRY(d_dist.alloc((size_t)P * 4));
    HIP_TRY(d_nodes.alloc(local.size() * 4));
    HIP_TRY(d_sum.alloc((size_t)n_groups * 8));
    HIP_TRY(d_unr.alloc((size_t)n_groups * 8));
    HIP_TRY(hipMemcpyAsync(d_grp.p, grp_ptr, (size_t)(n_groups + 1) * 8, hipMemcpyHostToDevice, g->st));
    if (M) HIP_TRY(hipMemcpyAsync(d_mem.p, mem.data(), (size_t)M * 4, hipMemcpyHostToDevice, g->st));
    HIP_TRY(hipMemcpyAsync(d_off.p, pair_off.data(), (size_t)(n_groups + 1) * 8, hipMemcpyHostToDevice, g->st));
    std::vector<int32_t> nodes(local.size(), -1);
    if (!local.empty()) {
        HIP_TRY(hipMemcpyAsync(d_local.p, local.data(), local.size() * 4, hipMemcpyHostToDevice, g->st));
        int32_t slots = 2;
        while (slots < g->local_capacity + g->local_capacity / 8) slots *= 2;
        HIP_TRY(nabo::paths_local_launch(g->rowptr.as<int32_t>(), g->col.as<int32_t>(), d_grp.as<int64_t>(), d_mem.as<int32_t>(),
                                         d_off.as<int64_t>(), d_local.as<int32_t>(), (int64_t)local.size(), slots,
                                         (int32_t)g->local_capacity, d_dist.as<int32_t>(), d_nodes.as<int32_t>(), g->st));
        HIP_TRY(hipMemcpyAsync(nodes.data(), d_nodes.p, local.size() * 4, hipMemcpyDeviceToHost, g->st));
        HIP_TRY(hipStreamSynchronize(g->st));
    }
    const double t1 = now_ms();
    g->ms[1] = t1 - t0;
    g->local_nodes.assign((size_t)n_groups, -1);
    std::vector<uint8_t> done((size_t)n_groups, 0);
    for (size_t i = 0; i < local.size(); ++i) {
        g->local_nodes[local[i]] = nodes[i];
        if (nodes[i] >= 0) {
            done[local[i]] = 1;
            ++g->stats[0];
        }
    }
    // global tier: every group with pairs the local tier did not answer
    std::vector<int32_t> src_id((size_t)g->n, -1), sources, uniq;
    std::vector<PathsPair> pairs;
    std::vector<int64_t> pair_sweep;
    for (int64_t i = 0; i < n_groups; ++i) {
        const int64_t a0 = grp_ptr[i], m = grp_ptr[i + 1] - a0;
        if (m < 2 || done[i]) continue;
        ++g->stats[1];
        // every pair needs one end that is a source: all distinct members but one must be
        uniq.assign(mem.begin() + a0, mem.begin() + a0 + m);
        std::sort(uniq.begin(), uniq.end());
        uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
        int64_t missing = 0;
        for (int32_t v : uniq) missing += src_id[v] < 0;
        for (int32_t v : uniq) {
            if (missing <= 1) break;
            if (src_id[v] < 0) {
                src_id[v] = (int32_t)sources.size();
                sources.push_back(v);
                --missing;
            }
        }
        for (int64_t x = 0; x < m; ++x)
            for (int64_t y = x + 1; y < m; ++y) {
                const int32_t a = mem[a0 + x], b = mem[a0 + y];
                const int64_t out = pair_off[i] + x * m - x * (x + 1) / 2 + (y - x - 1);
                if (a == b) {
                    pairs.push_back(PathsPair{0, -1, out});
                    pair_sweep.push_back(-1);
                    continue;
                }
                const int32_t s = src_id[a] >= 0 ? a : b, t = s == a ? b : a;
                pairs.push_back(PathsPair{t, src_id[s] % 64, out});
                pair_sweep.push_back(src_id[s] / 64);
            }
    }
    if (!pairs.empty()) {
        const int64_t n_sweeps = ((int64_t)sources.size() + 63) / 64;
        // bucket by sweep (counting sort); distance-0 pairs go last, outside every sweep's range
        std::vector<int64_t> cnt((size_t)n_sweeps + 1, 0);
        for (int64_t w : pair_sweep) ++cnt[w < 0 ? (size_t)n_sweeps : (size_t)w];
        std::vector<int64_t> start((size_t)n_sweeps + 2, 0);
        for (int64_t w = 0; w <= n_sweeps; ++w) start[w + 1] = start[w] + cnt[w];
        std::vector<PathsPair> sorted(pairs.size());
        std::vector<int64_t> fill(start.begin(), start.end() - 1);
        for (size_t p = 0; p < pairs.size(); ++p) sorted[fill[pair_sweep[p] < 0 ? n_sweeps : pair_sweep[p]]++] = pairs[p];
        const std::vector<int64_t> sweep_ptr(start.begin(), start.begin() + n_sweeps + 1);
        DevBuf d_pairs;
        HIP_TRY(d_pairs.alloc(sorted.size() * sizeof(PathsPair)));
        HIP_TRY(hipMemcpyAsync(d_pairs.p, sorted.data(), sorted.size() * sizeof(PathsPair), hipMemcpyHostToDevice, g->st));
        HIP_TRY(nabo::paths_prefill_launch(d_pairs.p, (int64_t)sorted.size(), d_dist.as<int32_t>(), g->st));
        if (n_sweeps > 0) {
            rc = run_global(g, sources, sweep_ptr, d_pairs.as<PathsPair>(), d_dist.as<int32_t>());
            if (rc) return rc;
        }
        HIP_TRY(hipStreamSynchronize(g->st));
    }
    const double t2 = now_ms();
    g->ms[2] = t2 - t1;
    HIP_TRY(nabo::paths_reduce_launch(d_off.as<int64_t>(), n_groups, d_dist.as<int32_t>(), d_sum.as<int64_t>(), d_unr.as<int64_t>(), g->st));
    if (n_groups) {
        HIP_TRY(hipMemcpyAsync(out_sum, d_sum.p, (size_t)n_groups * 8, hipMemcpyDeviceToHost, g->st));
        HIP_TRY(hipMemcpyAsync(out_unreached, d_unr.p, (size_t)n_groups * 8, hipMemcpyDeviceToHost, g->st));
    }
    if (out_pair_hops && P) HIP_TRY(hipMemcpyAsync(out_pair_hops, d_dist.p, (size_t)P * 4, hipMemcpyDeviceToHost, g->st));
    HIP_TRY(hipStreamSynchronize(g->st));
    g->ms[3] = now_ms() - t0;
    return NABO_OK;
}

int nabo_refgraph_last_stats(const nabo_refgraph *g, double ms[4], int64_t counters[4])
{
    if (!g || !ms || !counters) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    for (int i = 0; i < 4; ++i) {
        ms[i] = g->ms[i];
        counters[i] = g->stats[i];
    }
    return NABO_OK;
}

int nabo_refgraph_last_local_nodes(const nabo_refgraph *g, int64_t n_groups, int32_t *out)
{
    if (!g || (n_groups > 0 && !out)) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    if (n_groups != (int64_t)g->local_nodes.size())
        return nabo::api_fail(NABO_E_INVALID, "n_groups=%lld, the last call had %lld", (long long)n_groups, (long long)g->local_nodes.size());
    std::copy(g->local_nodes.begin(), g->local_nodes.end(), out);
    return NABO_OK;
}

int nabo_refgraph_set_levels(nabo_refgraph *g, int64_t n_sets, const int64_t *set_ptr, const int64_t *members, int32_t max_level,
                             int32_t *out_level)
{
    if (!g) return nabo::api_fail(NABO_E_INVALID, "NULL graph");
    if (n_sets < 0 || n_sets >= ((int64_t)1 << 31)) return nabo::api_fail(NABO_E_INVALID, "n_sets=%lld out of range", (long long)n_sets);
    int rc = nabo::check_csr_ptr("set_ptr", "set", n_sets, set_ptr);
    if (rc) return rc;
    const int64_t M = set_ptr[n_sets], n = g->n;
    if (M > 0 && !members) return nabo::api_fail(NABO_E_INVALID, "members is NULL");
    if (M >= ((int64_t)1 << 31)) return nabo::api_fail(NABO_E_UNSUPPORTED, "%lld members: fewer than 2^31 per call", (long long)M);
    if (n_sets > 0 && n > 0 && !out_level) return nabo::api_fail(NABO_E_INVALID, "out_level is NULL");
    std::vector<int32_t> node((size_t)M);
    std::vector<uint8_t> bit((size_t)M);
    for (int64_t s = 0; s < n_sets; ++s)
        for (int64_t i = set_ptr[s]; i < set_ptr[s + 1]; ++i) {
            if (members[i] < 0 || members[i] >= n)
                return nabo::api_fail(NABO_E_INVALID, "members[%lld] = %lld is not a node index in [0, %lld)", (long long)i, (long long)members[i], (long long)n);
            node[i] = (int32_t)members[i];
            bit[i] = (uint8_t)(s % 64);
        }
    if ((rc = use_device(g->device))) return rc;
    nabo::cluster_set_device_ms(1, 0.0);
    if (n_sets == 0 || n == 0) return NABO_OK;
    rc = ensure_global_state(g);
    if (rc) return rc;
    const int64_t per_sweep = std::min<int64_t>(64, n_sets);
    DevBuf d_node, d_bit, d_level;
    HIP_TRY(d_node.alloc((size_t)M * 4));
    HIP_TRY(d_bit.alloc((size_t)M));
    HIP_TRY(d_level.alloc((size_t)per_sweep * n * 4));
    if (M) {
        HIP_TRY(hipMemcpyAsync(d_node.p, node.data(), (size_t)M * 4, hipMemcpyHostToDevice, g->st));
        HIP_TRY(hipMemcpyAsync(d_bit.p, bit.data(), (size_t)M, hipMemcpyHostToDevice, g->st));
    }
    nabo::Events<2> E;
    HIP_TRY(E.create());
    int32_t *cur = g->cur.as<int32_t>(), *nxt_list = g->next_list.as<int32_t>();
    int64_t *cnt = g->counters.as<int64_t>();
    double device_ms = 0;
    for (int64_t s0 = 0; s0 < n_sets; s0 += 64) {
        const int64_t ns = std::min<int64_t>(64, n_sets - s0), m0 = set_ptr[s0], nm = set_ptr[s0 + ns] - m0;
        HIP_TRY(hipMemsetAsync(d_level.p, 0xFF, (size_t)ns * n * 4, g->st));
        HIP_TRY(hipEventRecord(E.ev[0], g->st));
        HIP_TRY(nabo::paths_seed_sets_launch(d_node.as<int32_t>() + m0, d_bit.as<uint8_t>() + m0, nm, n, g->visited.as<uint64_t>(),
                                             g->front.as<uint64_t>(), cur, g->touched.as<int32_t>(), cnt, d_level.as<int32_t>(), g->st));
        HIP_TRY(hipMemcpyAsync(g->host_counters, cnt + 3, 8, hipMemcpyDeviceToHost, g->st));
        HIP_TRY(hipStreamSynchronize(g->st));
        int64_t n_cur = g->host_counters[0];
        for (int32_t level = 1; n_cur > 0 && (max_level < 0 || level <= max_level); ++level) {
            HIP_TRY(nabo::paths_set_level_launch(g->rowptr.as<int32_t>(), g->col.as<int32_t>(), cur, nxt_list, g->visited.as<uint64_t>(),
                                                 g->front.as<uint64_t>(), g->nxt.as<uint64_t>(), g->touched.as<int32_t>(), n, level,
                                                 d_level.as<int32_t>(), cnt, n_cur, g->st));
            HIP_TRY(hipMemcpyAsync(g->host_counters, cnt, 8, hipMemcpyDeviceToHost, g->st));
            HIP_TRY(nabo::paths_advance_launch(cnt, g->st));
            HIP_TRY(hipStreamSynchronize(g->st));
            n_cur = g->host_counters[0];
            std::swap(cur, nxt_list);
        }
        HIP_TRY(nabo::paths_clear_launch(g->touched.as<int32_t>(), cnt, g->visited.as<uint64_t>(), g->front.as<uint64_t>(), g->st));
        HIP_TRY(hipEventRecord(E.ev[1], g->st));
        HIP_TRY(hipMemcpyAsync(out_level + s0 * n, d_level.p, (size_t)ns * n * 4, hipMemcpyDeviceToHost, g->st));
        HIP_TRY(hipStreamSynchronize(g->st));
        HIP_TRY(E.elapsed(0, 1, &device_ms));
    }
    nabo::cluster_set_device_ms(1, device_ms);
    return NABO_OK;
}

}  // extern "C"
