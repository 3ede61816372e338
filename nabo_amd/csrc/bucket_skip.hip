// bucket_skip.hip -- the two-level stream skips the sub-buckets a workgroup's rows cannot reach (gfx950; the rule, its
// allowance and the run list: bucket_skip.h).
//   references (behind the ordered copy, once per build): the groups' tiles, the buckets' means, the C x C unit directions
//     between them, and ymin [C][groups] -- per direction-from bucket the smallest projection of every group's references;
//   targets (per query, between the tournament and the main launch): one workgroup per workgroup of the main launch finds
//     how far its rows reach along the directions of their own buckets, tests every group and writes its run list.
// Everything is float64 up to the two directed roundings to fp32 of the header; nothing here waits for the device.
#include "launch.h"
#include "bucket_skip.h"

namespace nabo {

// fp32 <-> unsigned words that order as the floats do (for integer atomic minima / maxima)
__device__ inline uint32_t ord_of(float f)
{
    const uint32_t b = __float_as_uint(f);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ inline float ord_back(uint32_t u) { return __uint_as_float(u ^ ((u >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }

// group c = b * S + r: the positions of sub-bucket r of bucket b (sublay / subtot: the second sort's first positions and
// class sizes), or with S == 1 the bucket itself (lay: the layout of the full ordered copy)
__global__ __launch_bounds__(256) void bskip_groups_kernel(int C, int S, const int64_t *__restrict__ lay, const uint32_t *__restrict__ ref_cnt,
                                                           const int64_t *__restrict__ sublay, const uint32_t *__restrict__ subtot,
                                                           int32_t *__restrict__ first, int32_t *__restrict__ count,
                                                           int32_t *__restrict__ t0, int32_t *__restrict__ t1)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C * S) return;
    const int64_t f = S > 1 ? sublay[c] : lay[c];
    const int64_t n = S > 1 ? subtot[c] : ref_cnt[c];
    first[c] = (int32_t)f;
    count[c] = (int32_t)n;
    bskip_group_tiles(f, n, t0 + c, t1 + c);
}

// A tile of BSKIP_TILE cells in the packer's coordinates in LDS, [cell][BSKIP_MAX_DIM + 1] doubles (components past g: zero; one
// column of padding keeps the staging writes off one bank), and the lane's direction in registers: the inner product of a
// cell with the direction of lane b is BSKIP_MAX_DIM fused multiply-adds in index order on one broadcast LDS read each
// (the zero components add nothing: the sum is the header's bskip_dot).
constexpr int BSKIP_TILE = 64, BSKIP_LD = BSKIP_MAX_DIM + 1;
constexpr int BSKIP_MEAN_PARTS = 32;                     // slices of a bucket's positions, one workgroup each

// part [C][BSKIP_MEAN_PARTS][g]: sums of the packer's coordinates over a slice of bucket blockIdx.x's positions (32 lanes over
// the components, 8 rows at a time, each lane in position order); mean [C][g] from them, in slice order
__global__ __launch_bounds__(256) void bskip_mean_parts_kernel(const double *__restrict__ Y, const double *__restrict__ centre, double scale, int g,
                                                               int S, const uint32_t *__restrict__ ref_map, const int32_t *__restrict__ first,
                                                               const uint32_t *__restrict__ ref_cnt, double *__restrict__ part)
{
    __shared__ double rows8[8][BSKIP_MAX_DIM];
    const int b = blockIdx.x, lane = threadIdx.x & 31, row = threadIdx.x >> 5;
    const int64_t n = ref_cnt[b], per = (n + BSKIP_MEAN_PARTS - 1) / BSKIP_MEAN_PARTS;
    const int64_t p0 = first[b * S] + (int64_t)blockIdx.y * per, p1 = first[b * S] + (((int64_t)blockIdx.y + 1) * per < n ? ((int64_t)blockIdx.y + 1) * per : n);
    double acc[BSKIP_MAX_DIM / 32] = {0.0, 0.0};
    for (int64_t p = p0 + row; p < p1; p += 8) {
        const uint32_t j = ref_map[p];
        if (j == 0xFFFFFFFFu) continue;
#pragma unroll
        for (int e = 0; e < BSKIP_MAX_DIM / 32; ++e) {
            const int d = lane + 32 * e;
            if (d < g) acc[e] += bskip_coord(Y[(int64_t)j * g + d], centre[d], scale);
        }
    }
#pragma unroll
    for (int e = 0; e < BSKIP_MAX_DIM / 32; ++e) rows8[row][lane + 32 * e] = acc[e];
    __syncthreads();
    for (int d = threadIdx.x; d < g; d += 256) {
        double s = 0.0;
        for (int k = 0; k < 8; ++k) s += rows8[k][d];
        part[((int64_t)b * BSKIP_MEAN_PARTS + blockIdx.y) * g + d] = s;
    }
}
__global__ __launch_bounds__(64) void bskip_means_kernel(int g, const double *__restrict__ part, const uint32_t *__restrict__ ref_cnt,
                                                         double *__restrict__ mean)
{
    const int b = blockIdx.x, d = threadIdx.x;
    if (d >= g) return;
    double s = 0.0;
    for (int k = 0; k < BSKIP_MEAN_PARTS; ++k) s += part[((int64_t)b * BSKIP_MEAN_PARTS + k) * g + d];
    mean[(int64_t)b * g + d] = ref_cnt[b] > 0 ? s / (double)ref_cnt[b] : 0.0;
}

// u[b][b'] (bskip_direction), stored twice: by_from [b][d][b'] for the targets (a row's bucket is fixed, b' runs over the
// lanes) and by_to [b'][d][b] for the references
__global__ __launch_bounds__(64) void bskip_dirs_kernel(int C, int g, const double *__restrict__ mean, const uint32_t *__restrict__ ref_cnt,
                                                        double *__restrict__ by_from, double *__restrict__ by_to)
{
    const int w = blockIdx.x * 64 + threadIdx.x;
    if (w >= C * C) return;
    const int b = w / C, bp = w % C;
    // (bskip_direction's arithmetic, component by component: no array of the direction in a thread)
    const double *from = mean + (int64_t)b * g, *to = mean + (int64_t)bp * g;
    const double inv = bskip_direction_scale(g, from, to, b != bp && ref_cnt[b] > 0 && ref_cnt[bp] > 0);
    for (int d = 0; d < g; ++d) {
        const double u = bskip_direction_component(from[d], to[d], inv);
        by_from[((int64_t)b * g + d) * C + bp] = u;
        by_to[((int64_t)bp * g + d) * C + b] = u;
    }
}

// cells [p0, p1) of a map (0xFFFFFFFF: none -- a zero cell, flagged in live) into the tile, with their squared norms.  A thread
// takes one component of 16 cells: the 16 map entries, then the 16 gathers, are issued before anything waits for one; the
// norms are four partial sums of 16 components per cell, added in a fixed order (any order is inside the header's allowance).
__device__ inline void tile_stage(double *tile, double *norm2, uint8_t *live, const double *__restrict__ V, const double *__restrict__ centre, double scale,
                                  int g, const uint32_t *__restrict__ map, int64_t p0, int64_t p1)
{
    static_assert(BSKIP_TILE == 64 && BSKIP_MAX_DIM == 64, "256 threads: 64 components x 4 cells, 16 rounds");
    const int d = threadIdx.x & 63, c0 = threadIdx.x >> 6;
    const double cen = d < g ? centre[d] : 0.0;
    uint32_t j[16];
    double v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) j[k] = p0 + c0 + 4 * k < p1 ? map[p0 + c0 + 4 * k] : 0xFFFFFFFFu;
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = (j[k] != 0xFFFFFFFFu && d < g) ? V[(int64_t)j[k] * g + d] : cen;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        tile[(c0 + 4 * k) * BSKIP_LD + d] = (j[k] != 0xFFFFFFFFu && d < g) ? bskip_coord(v[k], cen, scale) : 0.0;
        if (d == 0) live[c0 + 4 * k] = j[k] != 0xFFFFFFFFu;
    }
    __syncthreads();
    {
        const int c = threadIdx.x >> 2, q = threadIdx.x & 3;
        double s2 = bskip_dot(BSKIP_MAX_DIM / 4, tile + c * BSKIP_LD + 16 * q, tile + c * BSKIP_LD + 16 * q);
        s2 += __shfl_xor(s2, 1, 64);
        s2 += __shfl_xor(s2, 2, 64);
        if (q == 0) norm2[c] = s2;
    }
    __syncthreads();
}

// the inner product of a cell of the tile with the lane's direction, in index order (the header's bskip_dot)
__device__ inline double tile_dot(const double *cell, const double (&u)[BSKIP_MAX_DIM])
{
    double s = 0.0;
#pragma unroll
    for (int d = 0; d < BSKIP_MAX_DIM; ++d) s = __builtin_fma(cell[d], u[d], s);
    return s;
}

// ymin [C][G]: one workgroup per group, its positions a tile at a time; thread = (slice of the tile's cells, direction-from
// bucket b), the direction u[b][b'] in its registers
__global__ __launch_bounds__(256) void bskip_ymin_kernel(const double *__restrict__ Y, const double *__restrict__ centre, double scale, int g, int C,
                                                         int S, int G, const uint32_t *__restrict__ ref_map, const int32_t *__restrict__ first,
                                                         const int32_t *__restrict__ count, const double *__restrict__ by_to,
                                                         float *__restrict__ ymin)
{
    __shared__ double tile[BSKIP_TILE * BSKIP_LD], norm2[BSKIP_TILE];
    __shared__ uint8_t live[BSKIP_TILE];
    __shared__ uint32_t smin[256];
    const int gi = blockIdx.x, bp = gi / S;
    const int slices = 256 / C, b = threadIdx.x % C, slice = threadIdx.x / C;
    const bool active = slice < slices;
    if (threadIdx.x < C) smin[threadIdx.x] = 0xFFFFFFFFu;
    double u[BSKIP_MAX_DIM];
#pragma unroll
    for (int d = 0; d < BSKIP_MAX_DIM; ++d) u[d] = (active && d < g) ? by_to[((int64_t)bp * g + d) * C + b] : 0.0;
    const int64_t p0 = first[gi], p1 = p0 + count[gi];
    double lo = __builtin_inf();
    bool any = false;
    for (int64_t p = p0; p < p1; p += BSKIP_TILE) {
        __syncthreads();
        tile_stage(tile, norm2, live, Y, centre, scale, g, ref_map, p, p1);
        for (int c = slice; active && c < BSKIP_TILE; c += slices) {
            if (!live[c]) continue;
            const double v = bskip_ref_value(tile_dot(tile + c * BSKIP_LD, u), bskip_ref_allow(norm2[c]));
            lo = v < lo ? v : lo;
            any = true;
        }
    }
    __syncthreads();
    if (any) atomicMin(&smin[b], ord_of(bskip_float_below(lo)));
    __syncthreads();
    if (threadIdx.x < C) ymin[(int64_t)threadIdx.x * G + gi] = smin[threadIdx.x] == 0xFFFFFFFFu ? __builtin_inff() : ord_back(smin[threadIdx.x]);
}

// One workgroup per workgroup of the ordered main launch (BSKIP_WG_ROWS positions from blockIdx.x * BSKIP_WG_ROWS on).
// row_map [position] = row of the launch (0xFFFFFFFF: padding), key [row] >> 16 = the row's bucket, tau [row] = its start
// threshold, X [row][g] the launch's rows as the packer read them.  Dynamic LDS: the bitmap of pairs of tiles, and behind it
// reach [BSKIP_OWN_MAX][C].
__global__ __launch_bounds__(256) void bskip_runs_kernel(const double *__restrict__ X, const double *__restrict__ centre, double scale, int g, int C,
                                                         int S, int G, const uint32_t *__restrict__ row_map, const uint32_t *__restrict__ key,
                                                         const float *__restrict__ tau, const double *__restrict__ by_from,
                                                         const float *__restrict__ ymin, const int32_t *__restrict__ t0,
                                                         const int32_t *__restrict__ t1, int32_t t_end, int32_t *__restrict__ runs_out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char bskip_smem[];
    uint32_t *words = reinterpret_cast<uint32_t *>(bskip_smem);
    __shared__ int own[BSKIP_OWN_MAX], veto;
    __shared__ double tile[BSKIP_TILE * BSKIP_LD], norm2[BSKIP_TILE], radius[BSKIP_TILE];
    __shared__ uint8_t live[BSKIP_TILE], has[BSKIP_OWN_MAX];
    __shared__ int slot[BSKIP_TILE];
    __shared__ unsigned long long scan[256];
    const int tid = threadIdx.x;
    const int nw = (int)bskip_bitmap_words(t_end);
    uint32_t *reach = words + nw;
    int32_t *runs = runs_out + (int64_t)blockIdx.x * BSKIP_RUN_INTS;
    if (tid < BSKIP_OWN_MAX) own[tid] = -1;
    if (tid == 0) veto = 0;
    for (int e = tid; e < BSKIP_OWN_MAX * C; e += 256) reach[e] = 0;
    for (int j = tid; j < nw; j += 256) words[j] = 0;
    // How far the rows of every own bucket reach towards every bucket b', a tile of rows at a time: thread = (slice of the
    // tile's rows, bucket b'), the direction u[own bucket][b'] in its registers while the tile's rows of that bucket pass.
    const int slices = 256 / C, bp_lane = tid % C, slice = tid / C;
    const bool active = slice < slices;
    const int64_t pos0 = (int64_t)blockIdx.x * BSKIP_WG_ROWS;
    // (g in a vector register: as wave-uniform conditions the 64 tests "d < g" of a direction's load are hoisted out of the
    // loops and hold 128 scalar registers for the length of the kernel)
    int gv = g;
    asm volatile("" : "+v"(gv));
#pragma unroll 1
    for (int chunk = 0; chunk < BSKIP_WG_ROWS / BSKIP_TILE; ++chunk) {
        __syncthreads();
        if (tid < BSKIP_OWN_MAX) has[tid] = 0;
        tile_stage(tile, norm2, live, X, centre, scale, g, row_map, pos0 + chunk * BSKIP_TILE, pos0 + BSKIP_WG_ROWS);
        if (tid < BSKIP_TILE) {
            int s = -1;
            if (live[tid]) {
                const uint32_t r = row_map[pos0 + chunk * BSKIP_TILE + tid], k = key[r];
                const int b = (int)(k >> 16);
                if (k != 0xFFFFFFFFu && b < C)
                    for (int c = 0; c < BSKIP_OWN_MAX && s < 0; ++c) {
                        const int cur = atomicCAS(&own[c], -1, b);
                        if (cur == -1 || cur == b) s = c;
                    }
                if (s < 0) veto = 1;               // (no bucket, or more own buckets than slots: nothing is skipped)
                else has[s] = 1;
                radius[tid] = bskip_row_radius(norm2[tid], tau[r]);
            }
            slot[tid] = s;
        }
        __syncthreads();
        if (veto) break;
        for (int s = 0; s < BSKIP_OWN_MAX && own[s] >= 0; ++s) {
            if (!has[s] || !active) continue;
            double u[BSKIP_MAX_DIM];
#pragma unroll
            for (int d = 0; d < BSKIP_MAX_DIM; ++d) u[d] = d < gv ? by_from[((int64_t)own[s] * g + d) * C + bp_lane] : 0.0;
            double hi = -__builtin_inf();
            for (int c = slice; c < BSKIP_TILE; c += slices)
                if (slot[c] == s) {
                    const double v = bskip_row_reach(tile_dot(tile + c * BSKIP_LD, u), radius[c]);
                    hi = v > hi ? v : hi;
                }
            if (hi > -__builtin_inf()) atomicMax(&reach[s * C + bp_lane], ord_of(bskip_float_above(hi)));
        }
    }
    __syncthreads();
    const bool off = veto != 0;
    // the groups: kept unless every own bucket's rows stay short of it; the own buckets' groups always
    for (int gi = tid; gi < G; gi += 256) {
        const int bp = gi / S;
        bool keep = off;
        for (int s = 0; s < BSKIP_OWN_MAX && !keep; ++s) {
            const int b = own[s];
            if (b < 0) continue;
            keep = b == bp || !bskip_row_allows(ymin[(int64_t)b * G + gi], ord_back(reach[s * C + bp]));
        }
        if (!keep) continue;
        int32_t p0, p1;
        bskip_group_pairs(t0[gi], t1[gi], t_end, &p0, &p1);
        for (int32_t p = p0; p < p1; ++p) atomicOr(&words[p >> 5], 1u << (p & 31));
    }
    __syncthreads();
    // the runs of the bitmap: every thread a stretch of words, a scan of the stretches' run starts and ends
    const int per = (nw + 255) / 256, j0 = tid * per, j1 = j0 + per < nw ? j0 + per : nw;
    unsigned long long mine = 0;
    for (int j = j0; j < j1; ++j) {
        mine += (unsigned long long)bskip_popcount(bskip_start_bits(words[j], j ? words[j - 1] >> 31 : 0));
        mine += (unsigned long long)bskip_popcount(bskip_end_bits(words[j], j + 1 < nw ? words[j + 1] : 0)) << 32;
    }
    scan[tid] = mine;
    __syncthreads();
    for (int step = 1; step < 256; step *= 2) {
        const unsigned long long add = tid >= step ? scan[tid - step] : 0;
        __syncthreads();
        scan[tid] += add;
        __syncthreads();
    }
    const int64_t nruns = (int64_t)(scan[255] & 0xFFFFFFFFull);
    int64_t ks = (int64_t)((scan[tid] - mine) & 0xFFFFFFFFull), ke = (int64_t)((scan[tid] - mine) >> 32);
    for (int j = j0; j < j1; ++j) {
        for (uint32_t m = bskip_start_bits(words[j], j ? words[j - 1] >> 31 : 0); m; m &= m - 1) bskip_emit_start(runs, BSKIP_RUN_CAP, ks++, 32 * (int64_t)j + (__ffs(m) - 1));
        for (uint32_t m = bskip_end_bits(words[j], j + 1 < nw ? words[j + 1] : 0); m; m &= m - 1) bskip_emit_end(runs, BSKIP_RUN_CAP, ke++, nruns, 32 * (int64_t)j + (__ffs(m) - 1));
    }
    if (tid == 0) bskip_emit_sentinel(runs, BSKIP_RUN_CAP, nruns);
}

size_t bskip_dir_bytes(int C, int g) { return (size_t)C * C * g * sizeof(double); }
size_t bskip_mean_part_bytes(int C, int g) { return (size_t)C * BSKIP_MEAN_PARTS * g * sizeof(double); }

// The reference side, behind the ordered copy on its stream.  lay / sublay / subtot: the layouts the copy was just sorted
// with (scratch that the next sort overwrites); the tables are the caller's, sized for C buckets, G = C * S groups.
hipError_t bskip_refs_launch(const double *Y, const double *centre, double scale, int g, int C, int S, const int64_t *lay,
                             const uint32_t *ref_cnt, const int64_t *sublay, const uint32_t *subtot, const uint32_t *ref_map,
                             int32_t *first, int32_t *count, int32_t *t0, int32_t *t1, double *mean_parts, double *mean, double *by_from,
                             double *by_to, float *ymin, hipStream_t st)
{
    const int G = C * S;
    if (g < 1 || g > BSKIP_MAX_DIM || C < 1 || C > 256 || S < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bskip_groups_kernel, dim3((G + 255) / 256), dim3(256), 0, st, C, S, lay, ref_cnt, sublay, subtot, first, count, t0, t1);
    hipLaunchKernelGGL(bskip_mean_parts_kernel, dim3(C, BSKIP_MEAN_PARTS), dim3(256), 0, st, Y, centre, scale, g, S, ref_map, first, ref_cnt, mean_parts);
    hipLaunchKernelGGL(bskip_means_kernel, dim3(C), dim3(64), 0, st, g, mean_parts, ref_cnt, mean);
    hipLaunchKernelGGL(bskip_dirs_kernel, dim3((C * C + 63) / 64), dim3(64), 0, st, C, g, mean, ref_cnt, by_from, by_to);
    hipLaunchKernelGGL(bskip_ymin_kernel, dim3(G), dim3(256), 0, st, Y, centre, scale, g, C, S, G, ref_map, first, count, by_to, ymin);
    return hipGetLastError();
}

// The target side: the run lists of `wgs` workgroups of the ordered main launch over a stream of t_end tiles
// (runs: wgs x BSKIP_RUN_INTS int32).
hipError_t bskip_runs_launch(const double *X, const double *centre, double scale, int g, int C, int S, const uint32_t *row_map,
                             const uint32_t *key, const float *tau, const double *by_from, const float *ymin, const int32_t *t0,
                             const int32_t *t1, int64_t t_end, int64_t wgs, int32_t *runs, hipStream_t st)
{
    if (g < 1 || g > BSKIP_MAX_DIM || C < 1 || C > 256 || S < 1 || t_end < 2 || (t_end & 1) || t_end > BSKIP_MAX_TILES || wgs < 1)
        return hipErrorInvalidValue;
    const size_t lds = ((size_t)bskip_bitmap_words((int32_t)t_end) + (size_t)BSKIP_OWN_MAX * C) * sizeof(uint32_t);
    // (static and dynamic LDS together stay below the 64 KB every launch may have unless the stream is very long or C is 256)
    if (lds > 24 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&bskip_runs_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(bskip_runs_kernel, dim3((unsigned)wgs), dim3(256), lds, st, X, centre, scale, g, C, S, C * S, row_map, key, tau, by_from,
                       ymin, t0, t1, (int32_t)t_end, runs);
    return hipGetLastError();
}

}  // namespace nabo
