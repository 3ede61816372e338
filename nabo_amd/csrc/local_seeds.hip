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
// The two-level stream (l2c_topk.hip) reads bucket-ordered copies of both sides made by the same sort; those copies are
// sorted once more inside their buckets, by sub-anchor (the sub-order: local_seeds.h, the kernels at the end of this file's
// device code).
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
// row_map [position] = i (the query side), or src_map [i] where the source is a sorted copy itself (the sub-order).
template <int KS>
__global__ __launch_bounds__(LSEED_BLOCK) void lseed_scatter_kernel(const unsigned char *__restrict__ src, int64_t ncell,
                                                                    const uint32_t *__restrict__ key, const uint32_t *__restrict__ blockoff,
                                                                    int64_t nblk, const int64_t *__restrict__ base, int cap,
                                                                    unsigned char *__restrict__ dst, uint32_t *__restrict__ row_map,
                                                                    const uint32_t *__restrict__ src_map)
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
    if (row_map) row_map[pos] = src_map ? src_map[i] : (uint32_t)i;
}

// ---- the sub-order inside the buckets (local_seeds.h): a second counting sort over the bucket-ordered copy ----------------

// sub [C][S][KS * 4] chunks and subf [C][S][KS * 32] floats: the component slots of bucket b's sub-anchors, cells of the
// bucket-ordered copy `pk` (caller order inside a bucket); zeros for a bucket without a sub-order
template <int KS>
__global__ void lseed_sub_anchors_kernel(const unsigned char *__restrict__ pk, const int64_t *__restrict__ base,
                                         const uint32_t *__restrict__ ref_cnt, int g, int C, int S, lh8 *__restrict__ sub,
                                         float *__restrict__ subf, bool two_level)
{
    constexpr int TB = 2 * KS * 1024;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= C * S * KS * 4) return;
    const int b = e / (S * KS * 4), j = (e / (KS * 4)) % S, s = (e / 4) % KS, lq = e % 4;
    lh8 v;
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = (_Float16)0.0f;
    const uint32_t cnt = ref_cnt[b];
    if (lseed_sub_applies(cnt, S)) {
        const int64_t cell = base[b] + lseed_sub_anchor_cell(cnt, S, j);
        v = *reinterpret_cast<const lh8 *>(pk + (cell >> 5) * TB + chunk_off<KS>((int)(cell & 31), s, lq));
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (!l2c_slot_is_comp(g, 32 * s + 8 * lq + q, two_level)) v[q] = (_Float16)0.0f;
    }
    sub[e] = v;
#pragma unroll
    for (int q = 0; q < 8; ++q) subf[((int64_t)(b * S + j) * KS + s) * 32 + lq * 8 + q] = (float)v[q];
}

// rank [C][S] and norm [C][S] = ||a||^2 of bucket blockIdx.x's sub-anchors: the ranking of local_seeds.h, one element per
// thread in the header's own order of operations
__global__ __launch_bounds__(LSEED_SUB_MAX_DIM) void lseed_sub_rank_kernel(int S, int dim, const float *__restrict__ subf, bool by_index,
                                                                           uint8_t *__restrict__ rank, float *__restrict__ norm)
{
    __shared__ double mean[LSEED_SUB_MAX_DIM], v[LSEED_SUB_MAX_DIM], w[LSEED_SUB_MAX_DIM], t[LSEED_MAX_SUB];
    const int tid = threadIdx.x;
    const float *pts = subf + (int64_t)blockIdx.x * S * dim;
    if (tid < S) {
        float s2 = 0.0f;
        for (int e = 0; e < dim; ++e) s2 = fmaf(pts[tid * dim + e], pts[tid * dim + e], s2);
        norm[blockIdx.x * S + tid] = s2;
    }
    if (by_index) {
        if (tid < S) rank[blockIdx.x * S + tid] = (uint8_t)tid;
        return;
    }
    if (tid < dim) {
        mean[tid] = lseed_sub_mean(S, dim, pts, tid);
        v[tid] = 1.0;
    }
    __syncthreads();
    for (int it = 0; it < LSEED_SUB_ITERS; ++it) {
        if (tid < S) t[tid] = lseed_sub_proj(dim, pts + tid * dim, mean, v);
        __syncthreads();
        if (tid < dim) w[tid] = lseed_sub_back(S, dim, pts, mean, t, tid);
        __syncthreads();
        const double ss = lseed_sub_sumsq(dim, w);          // (every thread: the same sum in the same order)
        if (!lseed_sub_dir_ok(ss)) break;
        if (tid < dim) v[tid] = w[tid] * (1.0 / sqrt(ss));
        __syncthreads();
    }
    __syncthreads();
    if (tid < S) t[tid] = lseed_sub_proj(dim, pts + tid * dim, mean, v);
    __syncthreads();
    if (tid < S) rank[blockIdx.x * S + tid] = (uint8_t)lseed_sub_rank_of(S, t, tid);
}

// One POSITION of the bucket-ordered copy per thread (map1 [position] = cell, 0xFFFFFFFF: padding; key1 [cell] >> 16 = its
// bucket): key2 [position] = (bucket * S + rank of the nearest sub-anchor) << 16 | rank among the block's earlier positions
// of that class, and the block's count per class in blockcnt [C * S][nblk] -- zero on entry, only the counts written.
template <int KS, bool IS_REF>
__global__ __launch_bounds__(LSEED_BLOCK) void lseed_sub_assign_kernel(const unsigned char *__restrict__ pk, int64_t npos,
                                                                       const uint32_t *__restrict__ map1, const uint32_t *__restrict__ key1,
                                                                       const lh8 *__restrict__ sub, const float *__restrict__ norm,
                                                                       const uint8_t *__restrict__ rank, const uint32_t *__restrict__ ref_cnt,
                                                                       int C, int S, uint32_t *__restrict__ key2,
                                                                       uint32_t *__restrict__ blockcnt, int64_t nblk)
{
    constexpr int TB = 2 * KS * 1024;
    extern __shared__ __attribute__((aligned(16))) unsigned char lseed_smem[];
    uint32_t *hist = reinterpret_cast<uint32_t *>(lseed_smem);          // [C * S]
    uint16_t *bk = reinterpret_cast<uint16_t *>(hist + C * S);          // [LSEED_BLOCK]
    const int tid = threadIdx.x;
    for (int c = tid; c < C * S; c += LSEED_BLOCK) hist[c] = 0;
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * LSEED_BLOCK + tid;
    const uint32_t cell = p < npos ? map1[p] : 0xFFFFFFFFu;
    const bool none = cell == 0xFFFFFFFFu;
    uint32_t cls = 0;
    if (!none) {
        const int b = (int)(key1[cell] >> 16);
        int r = 0;
        if (lseed_sub_applies(ref_cnt[b], S)) {
            const unsigned char *tp = pk + (p >> 5) * TB;
            const int c32 = (int)(p & 31);
            lh8 x[KS][4];
#pragma unroll
            for (int s = 0; s < KS; ++s)
#pragma unroll
                for (int lq = 0; lq < 4; ++lq) x[s][lq] = *reinterpret_cast<const lh8 *>(tp + chunk_off<KS>(c32, s, lq));
            float best = __builtin_inff();
            int bj = 0;
            for (int j = 0; j < S; ++j) {
                float d = 0.0f;
#pragma unroll
                for (int s = 0; s < KS; ++s)
#pragma unroll
                    for (int lq = 0; lq < 4; ++lq) {
                        const lh8 a = sub[((b * S + j) * KS + s) * 4 + lq];
                        const lh8 v = x[s][lq];
#pragma unroll
                        for (int q = 0; q < 8; q += 2)
                            d = __builtin_amdgcn_fdot2(lh2{a[q], a[q + 1]}, lh2{v[q], v[q + 1]}, d, false);
                    }
                const float sc = fmaf(IS_REF ? -2.0f : 1.0f, d, norm[b * S + j]);
                if (sc < best) { best = sc; bj = j; }
            }
            r = rank[b * S + bj];
        }
        cls = lseed_sub_key(b, S, r);
    }
    bk[tid] = none ? (uint16_t)0xFFFF : (uint16_t)cls;
    __syncthreads();
    if (!none) {
        atomicAdd(&hist[cls], 1u);
        uint32_t r = 0;
        for (int t = 0; t < tid; ++t) r += bk[t] == (uint16_t)cls;
        key2[p] = (cls << 16) | r;
    } else if (p < npos) {
        key2[p] = 0xFFFFFFFFu;
    }
    __syncthreads();
    for (int c = tid; c < C * S; c += LSEED_BLOCK)
        if (hist[c]) blockcnt[(int64_t)c * nblk + blockIdx.x] = hist[c];
}

// sublay [C * S]: first position of every (bucket, rank) class (lay: the buckets' layout, tot: the classes' sizes)
__global__ __launch_bounds__(256) void lseed_sub_layout_kernel(int C, int S, const int64_t *__restrict__ lay, const uint32_t *__restrict__ tot,
                                                               int64_t *__restrict__ sublay)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < C) lseed_sub_layout(b, S, lay, tot, sublay);
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
                       cap, dst, row_map, static_cast<const uint32_t *>(nullptr));
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

// ---- the sub-order (local_seeds.h): a bucket-ordered copy `pk` (map1 [position] = cell, key1 [cell] >> 16 = bucket) is
// sorted once more, inside its buckets, into the copy the stream reads ----------------------------------------------------

size_t lseed_sub_anchor_bytes(int kc, int C, int S) { return (size_t)C * S * (kc / 2) * 4 * 16; }
size_t lseed_sub_float_bytes(int kc, int C, int S) { return (size_t)C * S * (kc / 2) * 32 * sizeof(float); }

// The references' side, once per build: the sub-anchors of every bucket from the bucket-ordered copy (lay: its layout), their
// norms and ranks.  subf [C][S][16 kc] floats is scratch.
hipError_t lseed_sub_build_launch(int kc, const unsigned char *pk, const int64_t *lay, const uint32_t *ref_cnt, int g, int C, int S,
                                  bool by_index, void *anchors, float *subf, uint8_t *rank, float *norm, hipStream_t st, bool two_level)
{
    if (C < 1 || C > LSEED_MAX_ANCHORS || S < 2 || S > LSEED_MAX_SUB || kc < 2 || kc > 8 || (kc & 1)) return hipErrorInvalidValue;
    const int tot = C * S * (kc / 2) * 4;
    const dim3 grid((tot + 255) / 256);
    lh8 *a = reinterpret_cast<lh8 *>(anchors);
    switch (kc) {
    case 2: hipLaunchKernelGGL((lseed_sub_anchors_kernel<1>), grid, dim3(256), 0, st, pk, lay, ref_cnt, g, C, S, a, subf, two_level); break;
    case 4: hipLaunchKernelGGL((lseed_sub_anchors_kernel<2>), grid, dim3(256), 0, st, pk, lay, ref_cnt, g, C, S, a, subf, two_level); break;
    case 6: hipLaunchKernelGGL((lseed_sub_anchors_kernel<3>), grid, dim3(256), 0, st, pk, lay, ref_cnt, g, C, S, a, subf, two_level); break;
    default: hipLaunchKernelGGL((lseed_sub_anchors_kernel<4>), grid, dim3(256), 0, st, pk, lay, ref_cnt, g, C, S, a, subf, two_level); break;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lseed_sub_rank_kernel, dim3(C), dim3(LSEED_SUB_MAX_DIM), 0, st, S, (kc / 2) * 32, subf, by_index, rank, norm);
    return hipGetLastError();
}

template <int KS, bool IS_REF>
static hipError_t lseed_sub_assign_t(const unsigned char *pk, int64_t npos, const uint32_t *map1, const uint32_t *key1, const void *anchors,
                                     const float *norm, const uint8_t *rank, const uint32_t *ref_cnt, int C, int S, uint32_t *key2,
                                     uint32_t *blockcnt, hipStream_t st)
{
    const int64_t nblk = (npos + LSEED_BLOCK - 1) / LSEED_BLOCK;
    const size_t lds = (size_t)C * S * sizeof(uint32_t) + LSEED_BLOCK * sizeof(uint16_t);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&lseed_sub_assign_kernel<KS, IS_REF>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((lseed_sub_assign_kernel<KS, IS_REF>), dim3((unsigned)nblk), dim3(LSEED_BLOCK), lds, st, pk, npos, map1, key1,
                       reinterpret_cast<const lh8 *>(anchors), norm, rank, ref_cnt, C, S, key2, blockcnt, nblk);
    return hipGetLastError();
}

// The second sort: key2 [npos], blockcnt [C * S][blocks] (-> block offsets), tot [C * S], sublay [C * S] (first positions of
// the (bucket, rank) classes inside the buckets' layout `lay`).
hipError_t lseed_sub_sort_launch(int kc, bool is_ref, const unsigned char *pk, int64_t npos, const uint32_t *map1, const uint32_t *key1,
                                 const void *anchors, const float *norm, const uint8_t *rank, const uint32_t *ref_cnt, int C, int S,
                                 const int64_t *lay, uint32_t *key2, uint32_t *blockcnt, uint32_t *tot, int64_t *sublay, hipStream_t st)
{
    if (C < 1 || C > LSEED_MAX_ANCHORS || S < 2 || S > LSEED_MAX_SUB || npos < 1) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(blockcnt, 0, lseed_blockcnt_bytes(npos, C * S), st);
    if (e != hipSuccess) return e;
#define NABO_LSEED_SUB_ASSIGN(KSV)                                                                                                   \
    case 2 * KSV:                                                                                                                    \
        e = is_ref ? lseed_sub_assign_t<KSV, true>(pk, npos, map1, key1, anchors, norm, rank, ref_cnt, C, S, key2, blockcnt, st)     \
                   : lseed_sub_assign_t<KSV, false>(pk, npos, map1, key1, anchors, norm, rank, ref_cnt, C, S, key2, blockcnt, st);   \
        break;
    switch (kc) {
        NABO_LSEED_SUB_ASSIGN(1) NABO_LSEED_SUB_ASSIGN(2) NABO_LSEED_SUB_ASSIGN(3) NABO_LSEED_SUB_ASSIGN(4)
    default: return hipErrorInvalidValue;
    }
#undef NABO_LSEED_SUB_ASSIGN
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lseed_scan_kernel, dim3(C * S), dim3(256), 0, st, blockcnt, (npos + LSEED_BLOCK - 1) / LSEED_BLOCK, tot);
    hipLaunchKernelGGL(lseed_sub_layout_kernel, dim3((C + 255) / 256), dim3(256), 0, st, C, S, lay, tot, sublay);
    return hipGetLastError();
}

template <int KS>
static hipError_t lseed_sub_move_t(const unsigned char *src, int64_t npos, const uint32_t *map1, const uint32_t *key2,
                                   const uint32_t *blockoff, const int64_t *sublay, const unsigned char *pad_src, int64_t pad_cell, int C,
                                   const int64_t *lay, unsigned char *dst, uint32_t *dst_map, hipStream_t st)
{
    const int64_t nblk = (npos + LSEED_BLOCK - 1) / LSEED_BLOCK;
    hipLaunchKernelGGL((lseed_scatter_kernel<KS>), dim3((unsigned)nblk), dim3(LSEED_BLOCK), 0, st, src, npos, key2, blockoff, nblk, sublay,
                       0, dst, dst_map, map1);
    hipLaunchKernelGGL((lseed_pad_kernel<KS>), dim3(C + 1), dim3(LSEED_COL_ROWS), 0, st, pad_src, pad_cell, C, lay, dst);
    return hipGetLastError();
}

// The sub-ordered copy: position p of src to its position in dst, dst_map [position] = map1 [p]; the padding positions of the
// buckets' layout `lay` receive cell pad_cell of pad_src.
hipError_t lseed_sub_move_launch(int kc, const unsigned char *src, int64_t npos, const uint32_t *map1, const uint32_t *key2,
                                 const uint32_t *blockoff, const int64_t *sublay, const unsigned char *pad_src, int64_t pad_cell, int C,
                                 const int64_t *lay, unsigned char *dst, uint32_t *dst_map, hipStream_t st)
{
    switch (kc) {
    case 2: return lseed_sub_move_t<1>(src, npos, map1, key2, blockoff, sublay, pad_src, pad_cell, C, lay, dst, dst_map, st);
    case 4: return lseed_sub_move_t<2>(src, npos, map1, key2, blockoff, sublay, pad_src, pad_cell, C, lay, dst, dst_map, st);
    case 6: return lseed_sub_move_t<3>(src, npos, map1, key2, blockoff, sublay, pad_src, pad_cell, C, lay, dst, dst_map, st);
    case 8: return lseed_sub_move_t<4>(src, npos, map1, key2, blockoff, sublay, pad_src, pad_cell, C, lay, dst, dst_map, st);
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
