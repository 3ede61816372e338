// local_seeds.hip -- LOCAL tournament seeds for the one-product pass (gfx950): where the start thresholds of a row's list come
// from when the row's own neighbourhood is at hand.
//
// l2c_pre_kernel (l2c_topk.hip) bounds a row's lkeep-th smallest score by a tournament over some references; ANY references
// give a valid bound, and the closer they lie to the row the lower it is.  A random sample (the stream's first tiles) leaves
// ~lkeep ln(N / n0) list updates to the filter whatever its size; a sample from the row's own region of the data leaves a
// fraction of that.  The region is the cheapest partition there is: the nearest of C anchor cells (references at stride
// n / C), found on the packed f16 operands both sides already have.
//   references (once per set_ref / set_mask, behind the pack): assign -> stable counting sort by bucket -> the first `cap`
//     unmasked cells of every bucket are copied, cell by cell, into the bucket's run of whole tiles behind the packed stream
//     (masked and non-finite cells, +inf norm, are left out: they could not lower a seed);
//   targets (per query): assign -> the same sort -> a bucket-ordered copy of the packed target tiles and the map back to
//     the caller's rows, every bucket padded to whole columns of the tournament (local_seeds.h), one range per column.
// The filter itself reads the caller-order operands and the stream as before: only its start thresholds change.
// Everything is enqueued on the index's stream; nothing here waits for the device.
#include "local_seeds.h"

#include "knn_common.h"
#include "l2c_slots.h"
#include "launch.h"

namespace nabo {

typedef _Float16 lh2 __attribute__((ext_vector_type(2)));
typedef _Float16 lh8 __attribute__((ext_vector_type(8)));

// byte offset of chunk (s, lq) of cell c inside its tile (pack_ctiles_kernel, L16 layout: register h KS + s, lane
// 16 lq + (c & 15), h = c >> 4; 16 bytes = slots 32 s + 8 lq .. + 8)
template <int KS>
__device__ __forceinline__ int chunk_off(int c, int s, int lq)
{
    return ((((c >> 4) * KS + s) * 64) + lq * 16 + (c & 15)) * 16;
}

template <int KS>
__device__ __forceinline__ void cell_copy(const unsigned char *__restrict__ src, int64_t si, unsigned char *__restrict__ dst, int64_t di)
{
    constexpr int TB = 2 * KS * 1024;
    const unsigned char *sp = src + (si >> 5) * TB;
    unsigned char *dp = dst + (di >> 5) * TB;
    uint4 v[KS][4];
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int lq = 0; lq < 4; ++lq) v[s][lq] = *reinterpret_cast<const uint4 *>(sp + chunk_off<KS>((int)(si & 31), s, lq));
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int lq = 0; lq < 4; ++lq) *reinterpret_cast<uint4 *>(dp + chunk_off<KS>((int)(di & 31), s, lq)) = v[s][lq];
}

// anchors [C][KS][4] chunks: the component slots of reference cell c * stride, every other slot (norms, error, tail
// bounds) zero.  two_level: the operands are in the two-level slot order (l2c_slots.h).
template <int KS>
__global__ void lseed_anchors_kernel(const unsigned char *__restrict__ Ypk, int64_t stride, int g, int C, lh8 *__restrict__ anchors,
                                     bool two_level)
{
    constexpr int TB = 2 * KS * 1024;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= C * KS * 4) return;
    const int c = e / (KS * 4), s = (e / 4) % KS, lq = e % 4;
    const int64_t cell = (int64_t)c * stride;
    lh8 v = *reinterpret_cast<const lh8 *>(Ypk + (cell >> 5) * TB + chunk_off<KS>((int)(cell & 31), s, lq));
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (!l2c_slot_is_comp(g, 32 * s + 8 * lq + j, two_level)) v[j] = (_Float16)0.0f;
    anchors[e] = v;
}

// One cell per thread: its bucket = the anchor of smallest ||a||^2 - 2 a.v over the f16 component slots (fp32 sums in a
// fixed order; ties to the lowest anchor), key = bucket << 16 | rank among the block's earlier cells of that bucket
// (0xFFFFFFFF: no bucket -- a reference with +inf norm), and the block's count per bucket, blockcnt [C][nblk].
// Targets hold -2 v (IS_REF = false).
template <int KS, bool IS_REF>
__global__ __launch_bounds__(LSEED_BLOCK) void lseed_assign_kernel(const unsigned char *__restrict__ pk, int64_t ncell, int g,
                                                                   const lh8 *__restrict__ anchors, int C,
                                                                   uint32_t *__restrict__ key, uint32_t *__restrict__ blockcnt,
                                                                   int64_t nblk, bool two_level)
{
    constexpr int TB = 2 * KS * 1024;
    extern __shared__ __attribute__((aligned(16))) unsigned char lseed_smem[];
    lh8 *A = reinterpret_cast<lh8 *>(lseed_smem);                       // [C][KS * 4]
    float *an = reinterpret_cast<float *>(A + C * KS * 4);              // [C]
    uint32_t *hist = reinterpret_cast<uint32_t *>(an + C);              // [C]
    uint16_t *bk = reinterpret_cast<uint16_t *>(hist + C);              // [LSEED_BLOCK]
    const int tid = threadIdx.x;
    for (int e = tid; e < C * KS * 4; e += LSEED_BLOCK) A[e] = anchors[e];
    for (int c = tid; c < C; c += LSEED_BLOCK) hist[c] = 0;
    __syncthreads();
    for (int c = tid; c < C; c += LSEED_BLOCK) {
        float s2 = 0.0f;
        for (int e = 0; e < KS * 4; ++e) {
            const lh8 a = A[c * KS * 4 + e];
#pragma unroll
            for (int j = 0; j < 8; ++j) s2 = fmaf((float)a[j], (float)a[j], s2);
        }
        an[c] = s2;
    }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * LSEED_BLOCK + tid;
    const bool live = i < ncell;
    const int64_t ci = live ? i : 0;
    const unsigned char *tp = pk + (ci >> 5) * TB;
    const int c32 = (int)(ci & 31);
    lh8 x[KS][4];
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int lq = 0; lq < 4; ++lq) x[s][lq] = *reinterpret_cast<const lh8 *>(tp + chunk_off<KS>(c32, s, lq));
    bool none = !live;
    if (IS_REF) {           // the high part of the norm (slot g, or the two-level order's): +inf for a masked, non-finite or padding cell
        const int ns = l2c_norm_slot(g, two_level);
        const _Float16 nh = *reinterpret_cast<const _Float16 *>(tp + chunk_off<KS>(c32, ns >> 5, (ns & 31) >> 3) + 2 * (ns & 7));
        none = none || !((float)nh < __builtin_inff());
    }
    float best = __builtin_inff();
    int bb = 0;
    for (int c = 0; c < C; ++c) {
        float d = 0.0f;
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int lq = 0; lq < 4; ++lq) {
                const lh8 a = A[(c * KS + s) * 4 + lq];
                const lh8 v = x[s][lq];
#pragma unroll
                for (int j = 0; j < 8; j += 2)
                    d = __builtin_amdgcn_fdot2(lh2{a[j], a[j + 1]}, lh2{v[j], v[j + 1]}, d, false);
            }
        const float sc = fmaf(IS_REF ? -2.0f : 1.0f, d, an[c]);
        if (sc < best) { best = sc; bb = c; }
    }
    bk[tid] = none ? (uint16_t)0xFFFF : (uint16_t)bb;
    __syncthreads();
    if (!none) {
        atomicAdd(&hist[bb], 1u);
        uint32_t r = 0;
        for (int t = 0; t < tid; ++t) r += bk[t] == (uint16_t)bb;
        key[i] = ((uint32_t)bb << 16) | r;
    } else if (live) {
        key[i] = 0xFFFFFFFFu;
    }
    __syncthreads();
    for (int c = tid; c < C; c += LSEED_BLOCK) blockcnt[(int64_t)c * nblk + blockIdx.x] = hist[c];
}

// blockcnt [C][nblk] -> exclusive prefix over the blocks, in place; tot [C] = cells per bucket.  One workgroup per bucket.
__global__ __launch_bounds__(256) void lseed_scan_kernel(uint32_t *__restrict__ blockcnt, int64_t nblk, uint32_t *__restrict__ tot)
{
    __shared__ uint32_t part[256];
    uint32_t *p = blockcnt + (int64_t)blockIdx.x * nblk;
    const int tid = threadIdx.x;
    const int64_t per = (nblk + 255) / 256;
    const int64_t lo = tid * per < nblk ? tid * per : nblk, hi = lo + per < nblk ? lo + per : nblk;
    uint32_t s = 0;
    for (int64_t j = lo; j < hi; ++j) s += p[j];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0;
        for (int t = 0; t < 256; ++t) {
            const uint32_t v = part[t];
            part[t] = run;
            run += v;
        }
        tot[blockIdx.x] = run;
    }
    __syncthreads();
    uint32_t run = part[tid];
    for (int64_t j = lo; j < hi; ++j) {
        const uint32_t v = p[j];
        p[j] = run;
        run += v;
    }
}

// lay = base [C + 1] | padb [C + 1] | pade [C + 1] (local_seeds.h); the query side also writes its columns' ranges
__global__ __launch_bounds__(256) void lseed_layout_kernel(int C, const uint32_t *__restrict__ ref_cnt, const uint32_t *__restrict__ row_cnt,
                                                           int cap, int lkeep, int tile0, LseedRange rest, int64_t *__restrict__ lay,
                                                           LseedRange *__restrict__ ranges, int64_t ncol)
{
    int64_t *base = lay, *padb = lay + (C + 1), *pade = lay + 2 * (C + 1);
    if (threadIdx.x == 0) {
        if (!row_cnt && cap == 0) lseed_layout_full(C, ref_cnt, base, padb, pade);      // the full ordered copy of the references
        else lseed_layout(C, ref_cnt, row_cnt, cap, lkeep, tile0, base, padb, pade);
    }
    __syncthreads();
    if (!ranges) return;
    for (int b = threadIdx.x; b <= C; b += 256) lseed_fill_columns(b, C, ref_cnt, cap, lkeep, tile0, rest, base, pade, ranges, ncol);
}

// lay (of the full ordered copy) -> the buckets' ends in tiles
__global__ __launch_bounds__(64) void lseed_ends_kernel(int C, const int64_t *__restrict__ lay, int32_t *__restrict__ end)
{
    if (threadIdx.x == 0) lseed_bucket_ends(C, lay + 2 * (C + 1), end);
}

// cell i -> position base[bucket] + (its block's offset + its rank); a reference beyond its bucket's cap stays behind.
// row_map [position] = i (the query side).
template <int KS>
__global__ __launch_bounds__(LSEED_BLOCK) void lseed_scatter_kernel(const unsigned char *__restrict__ src, int64_t ncell,
                                                                    const uint32_t *__restrict__ key, const uint32_t *__restrict__ blockoff,
                                                                    int64_t nblk, const int64_t *__restrict__ base, int cap,
                                                                    unsigned char *__restrict__ dst, uint32_t *__restrict__ row_map)
{
    const int64_t i = (int64_t)blockIdx.x * LSEED_BLOCK + threadIdx.x;
    if (i >= ncell) return;
    const uint32_t k = key[i];
    if (k == 0xFFFFFFFFu) return;
    const int b = (int)(k >> 16);
    const int64_t in_bucket = (int64_t)blockoff[(int64_t)b * nblk + blockIdx.x] + (k & 0xFFFFu);
    if (cap > 0 && in_bucket >= cap) return;
    const int64_t pos = base[b] + in_bucket;
    cell_copy<KS>(src, i, dst, pos);
    if (row_map) row_map[pos] = (uint32_t)i;
}

// the padding positions of class blockIdx.x receive cell `pad_cell` of src (an all-padding reference; any target row)
template <int KS>
__global__ __launch_bounds__(LSEED_COL_ROWS) void lseed_pad_kernel(const unsigned char *__restrict__ src, int64_t pad_cell, int C,
                                                                   const int64_t *__restrict__ lay, unsigned char *__restrict__ dst)
{
    const int64_t p = lay[(C + 1) + blockIdx.x] + threadIdx.x;
    if (p < lay[2 * (C + 1) + blockIdx.x]) cell_copy<KS>(src, pad_cell, dst, p);
}

// every cell of dst [0, ncell) receives cell `pad_cell` of src
template <int KS>
__global__ __launch_bounds__(256) void lseed_fill_kernel(const unsigned char *__restrict__ src, int64_t pad_cell, int64_t ncell,
                                                         unsigned char *__restrict__ dst)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < ncell) cell_copy<KS>(src, pad_cell, dst, i);
}

size_t lseed_key_bytes(int64_t ncell) { return (size_t)ncell * sizeof(uint32_t); }
size_t lseed_blockcnt_bytes(int64_t ncell, int C) { return (size_t)((ncell + LSEED_BLOCK - 1) / LSEED_BLOCK) * C * sizeof(uint32_t); }
size_t lseed_layout_bytes(int C) { return (size_t)3 * (C + 1) * sizeof(int64_t); }
size_t lseed_anchor_bytes(int kc, int C) { return (size_t)C * (kc / 2) * 4 * 16; }

template <int KS>
static hipError_t lseed_anchors_t(const unsigned char *Ypk, int64_t n, int g, int C, void *anchors, hipStream_t st, bool two_level)
{
    const int tot = C * KS * 4;
    hipLaunchKernelGGL((lseed_anchors_kernel<KS>), dim3((tot + 255) / 256), dim3(256), 0, st, Ypk, n / C, g, C, reinterpret_cast<lh8 *>(anchors),
                       two_level);
    return hipGetLastError();
}

hipError_t lseed_anchors_launch(int kc, const unsigned char *Ypk, int64_t n, int g, int C, void *anchors, hipStream_t st, bool two_level)
{
    if (C < 1 || C > LSEED_MAX_ANCHORS || n < C || (two_level && (kc != 4 || !l2c_slots_fit(g)))) return hipErrorInvalidValue;
    switch (kc) {
    case 2: return lseed_anchors_t<1>(Ypk, n, g, C, anchors, st, two_level);
    case 4: return lseed_anchors_t<2>(Ypk, n, g, C, anchors, st, two_level);
    case 6: return lseed_anchors_t<3>(Ypk, n, g, C, anchors, st, two_level);
    case 8: return lseed_anchors_t<4>(Ypk, n, g, C, anchors, st, two_level);
    default: return hipErrorInvalidValue;
    }
}

template <int KS, bool IS_REF>
static hipError_t lseed_assign_t(const unsigned char *pk, int64_t ncell, int g, const void *anchors, int C, uint32_t *key,
                                 uint32_t *blockcnt, hipStream_t st, bool two_level)
{
    const int64_t nblk = (ncell + LSEED_BLOCK - 1) / LSEED_BLOCK;
    const size_t lds = (size_t)C * KS * 4 * 16 + (size_t)C * 8 + LSEED_BLOCK * sizeof(uint16_t);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&lseed_assign_kernel<KS, IS_REF>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((lseed_assign_kernel<KS, IS_REF>), dim3((unsigned)nblk), dim3(LSEED_BLOCK), lds, st, pk, ncell, g,
                       reinterpret_cast<const lh8 *>(anchors), C, key, blockcnt, nblk, two_level);
    return hipGetLastError();
}

// Sort `ncell` packed cells (tile 0 of pk holds cell 0) by bucket: key [ncell], blockcnt [C][blocks] (-> block offsets),
// tot [C].  is_ref: cells with +inf norm get no bucket.
hipError_t lseed_sort_launch(int kc, bool is_ref, const unsigned char *pk, int64_t ncell, int g, const void *anchors, int C,
                             uint32_t *key, uint32_t *blockcnt, uint32_t *tot, hipStream_t st, bool two_level)
{
    if (C < 1 || C > LSEED_MAX_ANCHORS || ncell < 1 || (two_level && (kc != 4 || !l2c_slots_fit(g)))) return hipErrorInvalidValue;
    hipError_t e;
#define NABO_LSEED_ASSIGN(KSV)                                                                                                       \
    case 2 * KSV:                                                                                                                    \
        e = is_ref ? lseed_assign_t<KSV, true>(pk, ncell, g, anchors, C, key, blockcnt, st, two_level)                               \
                   : lseed_assign_t<KSV, false>(pk, ncell, g, anchors, C, key, blockcnt, st, two_level);                             \
        break;
    switch (kc) {
        NABO_LSEED_ASSIGN(1) NABO_LSEED_ASSIGN(2) NABO_LSEED_ASSIGN(3) NABO_LSEED_ASSIGN(4)
    default: return hipErrorInvalidValue;
    }
#undef NABO_LSEED_ASSIGN
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lseed_scan_kernel, dim3(C), dim3(256), 0, st, blockcnt, (ncell + LSEED_BLOCK - 1) / LSEED_BLOCK, tot);
    return hipGetLastError();
}

// row_cnt == nullptr: the reference side (ranges unused); with cap == 0 the layout of the full ordered copy
hipError_t lseed_layout_launch(int C, const uint32_t *ref_cnt, const uint32_t *row_cnt, int cap, int lkeep, int tile0,
                               const int rest[4], int64_t *lay, int *ranges, int64_t ncol, hipStream_t st)
{
    const LseedRange r = {rest[0], rest[1], rest[2], rest[3]};
    hipLaunchKernelGGL(lseed_layout_kernel, dim3(1), dim3(256), 0, st, C, ref_cnt, row_cnt, cap, lkeep, tile0, r, lay,
                       reinterpret_cast<LseedRange *>(ranges), ncol);
    return hipGetLastError();
}

// end [C]: the buckets' ends in tiles, from the layout lseed_layout_launch made of the full ordered copy (cap == 0)
hipError_t lseed_ends_launch(int C, const int64_t *lay, int32_t *end, hipStream_t st)
{
    hipLaunchKernelGGL(lseed_ends_kernel, dim3(1), dim3(64), 0, st, C, lay, end);
    return hipGetLastError();
}

template <int KS>
static hipError_t lseed_move_t(const unsigned char *src, int64_t ncell, const uint32_t *key, const uint32_t *blockoff, int C,
                               const int64_t *lay, int cap, int64_t pad_cell, unsigned char *dst, uint32_t *row_map, hipStream_t st)
{
    const int64_t nblk = (ncell + LSEED_BLOCK - 1) / LSEED_BLOCK;
    hipLaunchKernelGGL((lseed_scatter_kernel<KS>), dim3((unsigned)nblk), dim3(LSEED_BLOCK), 0, st, src, ncell, key, blockoff, nblk, lay,
                       cap, dst, row_map);
    hipLaunchKernelGGL((lseed_pad_kernel<KS>), dim3(C + 1), dim3(LSEED_COL_ROWS), 0, st, src, pad_cell, C, lay, dst);
    return hipGetLastError();
}

// The sorted copy: cell i of src to its position in dst (cap > 0: at most cap cells per bucket), padding positions filled
// with cell pad_cell of src, row_map [position] = i where one is given (the caller fills it with 0xFFFFFFFF first).
hipError_t lseed_move_launch(int kc, const unsigned char *src, int64_t ncell, const uint32_t *key, const uint32_t *blockoff, int C,
                             const int64_t *lay, int cap, int64_t pad_cell, unsigned char *dst, uint32_t *row_map, hipStream_t st)
{
    switch (kc) {
    case 2: return lseed_move_t<1>(src, ncell, key, blockoff, C, lay, cap, pad_cell, dst, row_map, st);
    case 4: return lseed_move_t<2>(src, ncell, key, blockoff, C, lay, cap, pad_cell, dst, row_map, st);
    case 6: return lseed_move_t<3>(src, ncell, key, blockoff, C, lay, cap, pad_cell, dst, row_map, st);
    case 8: return lseed_move_t<4>(src, ncell, key, blockoff, C, lay, cap, pad_cell, dst, row_map, st);
    default: return hipErrorInvalidValue;
    }
}

// dst [0, ncell) filled with cell pad_cell of src (the full ordered copy starts as padding cells)
hipError_t lseed_fill_launch(int kc, const unsigned char *src, int64_t pad_cell, unsigned char *dst, int64_t ncell, hipStream_t st)
{
    const dim3 grid((unsigned)((ncell + 255) / 256));
    switch (kc) {
    case 2: hipLaunchKernelGGL((lseed_fill_kernel<1>), grid, dim3(256), 0, st, src, pad_cell, ncell, dst); break;
    case 4: hipLaunchKernelGGL((lseed_fill_kernel<2>), grid, dim3(256), 0, st, src, pad_cell, ncell, dst); break;
    case 6: hipLaunchKernelGGL((lseed_fill_kernel<3>), grid, dim3(256), 0, st, src, pad_cell, ncell, dst); break;
    case 8: hipLaunchKernelGGL((lseed_fill_kernel<4>), grid, dim3(256), 0, st, src, pad_cell, ncell, dst); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace nabo
