// local_seeds.h -- the layout rules of the LOCAL tournament seeds (local_seeds.hip), as functions the device kernels and the
// host share: tests/test_local_seeds_cpu.py compiles this header for the host and checks the rules without a GPU.
//
// The references are cut into C buckets (nearest of C anchor cells); bucket b owns a fixed slot of cap / 32 tiles behind the
// packed reference stream and fills it with its first `cap` unmasked cells.  A query sorts its rows by bucket, pads every
// bucket's rows to whole columns of LSEED_COL_ROWS rows, and l2c_pre_kernel runs each column's tournament over its bucket's
// run instead of the stream's first tiles.  Buckets whose run is too short for a tournament form one REST class at the
// end: its columns keep the stream-prefix tournament.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define NABO_HD __host__ __device__
#else
#define NABO_HD
#endif

namespace nabo {

constexpr int LSEED_MAX_ANCHORS = 256;
constexpr int LSEED_MAX_CAP = 32768;
constexpr int LSEED_COL_ROWS = 128;     // a whole number of waves of every l2c_pre_kernel instantiation (128 or 64 rows)
constexpr int64_t LSEED_MIN_REFS = 1 << 18, LSEED_MIN_ROWS = 1 << 16;     // where option local_seeds = 1 switches them on
constexpr int LSEED_BLOCK = 256;        // cells per workgroup of the assignment: the unit of the counting sort's block offsets

struct LseedRange { int t0, t1, pt, gt; };      // one int4 of l2c_pre_kernel's `ranges`: first tile, end tile, tournament tiles, tiles per group

// The tournament over a bucket's run of T tiles: ALL of it (the cap is the cost knob: a run costs a row what the same
// number of stream tiles does, l2c_pre_plan, but its cells are the row's neighbourhood), in groups of gt tiles as
// l2c_pre_plan cuts them; pt is rounded UP to whole groups -- past the run's end the kernel reads the all-padding tile.
// pt = 0: fewer than 3 q groups of two tiles, the bound would be loose (l2c_pre_plan's rule) -- the bucket joins the rest class.
NABO_HD inline void lseed_tournament(int lkeep, int T, int *pt, int *gt)
{
    const int q = (lkeep + 3) / 4;
    *pt = 0;
    *gt = 2;
    if (T < 6 * q) return;
    int g2 = T / (8 * q);
    g2 = g2 < 2 ? 2 : (g2 > 8 ? 8 : g2 & ~1);
    *gt = g2;
    *pt = (T + g2 - 1) / g2 * g2;
}

NABO_HD inline LseedRange lseed_bucket_range(int b, uint32_t ref_cnt, int cap, int lkeep, int tile0)
{
    const int kept = ref_cnt < (uint32_t)cap ? (int)ref_cnt : cap;
    const int T = (kept + 31) / 32;
    LseedRange r = {0, 0, 0, 0};
    lseed_tournament(lkeep, T, &r.pt, &r.gt);
    if (r.pt == 0) return LseedRange{0, 0, 0, 0};
    r.t0 = tile0 + b * (cap / 32);
    r.t1 = r.t0 + T;
    return r;
}

// Positions of the sorted cells.  base[b]: first position of bucket b's cells (base[C]: of the rest class);
// [padb[b], pade[b]): the padding positions behind them (entry C: behind the rest class).
//   row_cnt == nullptr -- the REFERENCE side: fixed slots of `cap` cells, the last tile of a run padded;
//   otherwise the QUERY side: buckets with a tournament first, each padded to whole columns, then the rows of all other
//   buckets back to back as the rest class, padded once.
NABO_HD inline void lseed_layout(int C, const uint32_t *ref_cnt, const uint32_t *row_cnt, int cap, int lkeep, int tile0,
                                 int64_t *base, int64_t *padb, int64_t *pade)
{
    if (!row_cnt) {
        for (int b = 0; b < C; ++b) {
            const int64_t kept = ref_cnt[b] < (uint32_t)cap ? ref_cnt[b] : cap;
            base[b] = (int64_t)b * cap;
            padb[b] = base[b] + kept;
            pade[b] = base[b] + (kept + 31) / 32 * 32;
        }
        base[C] = (int64_t)C * cap;
        padb[C] = pade[C] = 0;
        return;
    }
    int64_t pos = 0;
    for (int b = 0; b < C; ++b) {
        if (lseed_bucket_range(b, ref_cnt[b], cap, lkeep, tile0).pt == 0) continue;
        base[b] = pos;
        padb[b] = pos + row_cnt[b];
        pos += ((int64_t)row_cnt[b] + LSEED_COL_ROWS - 1) / LSEED_COL_ROWS * LSEED_COL_ROWS;
        pade[b] = pos;
    }
    base[C] = pos;
    for (int b = 0; b < C; ++b) {
        if (lseed_bucket_range(b, ref_cnt[b], cap, lkeep, tile0).pt != 0) continue;
        base[b] = pos;
        padb[b] = pade[b] = 0;
        pos += row_cnt[b];
    }
    padb[C] = pos;
    pade[C] = base[C] + (pos - base[C] + LSEED_COL_ROWS - 1) / LSEED_COL_ROWS * LSEED_COL_ROWS;
}

// The FULL bucket-ordered copy of the references (the two-level stream of l2c_topk.hip): every unmasked cell of bucket b at
// base[b] + its rank, buckets back to back in whole tiles, [padb[b], pade[b]) the padding of a bucket's last tile.  The
// copy holds at most ref_tiles + C tiles (lseed_ordered_tiles; what the buckets leave unused is padding cells too).
NABO_HD inline void lseed_layout_full(int C, const uint32_t *ref_cnt, int64_t *base, int64_t *padb, int64_t *pade)
{
    int64_t pos = 0;
    for (int b = 0; b < C; ++b) {
        base[b] = pos;
        padb[b] = pos + ref_cnt[b];
        pos += ((int64_t)ref_cnt[b] + 31) / 32 * 32;
        pade[b] = pos;
    }
    base[C] = pos;
    padb[C] = pade[C] = 0;
}
// The buckets' ENDS in tiles of the full ordered copy (pade of lseed_layout_full): end[b] = first tile behind bucket b --
// non-decreasing, an empty bucket repeats its predecessor's end, the last one <= lseed_ordered_tiles.  The table the
// filter's mode control walks (l2c_topk.hip).
NABO_HD inline void lseed_bucket_ends(int C, const int64_t *pade, int32_t *end)
{
    for (int b = 0; b < C; ++b) end[b] = (int32_t)(pade[b] / 32);
}
// tiles the ordered stream runs over (even: the filter's loop runs in twos), without the two padding tiles behind them
inline int64_t lseed_ordered_tiles(int64_t ref_tiles, int C) { return (ref_tiles + C + 1) / 2 * 2; }

// ---- the SUB-ORDER of the two-level stream's copies: where a cell lies INSIDE its bucket -------------------------------
// Both bucket-ordered copies (references: yord; targets: xpre) keep every bucket's range and sort the cells inside it by
// (sub-rank, caller order).  A bucket with at least S unmasked references has S SUB-ANCHORS: its unmasked references number
// j * (count / S), j < S, in caller order.  A cell's sub-anchor is the nearest one (||a||^2 - 2 a.v on the component slots,
// fp32, ties to the lowest j); the sub-anchors are RANKED along the first principal direction of the S of them (power
// iteration from the all-ones vector, LSEED_SUB_ITERS steps in float64, equal projections by j), so that neighbours in the
// stream are neighbours in space.  Buckets with fewer than S unmasked references keep caller order (every cell rank 0).
// Targets use the references' sub-anchors and ranks.  Any order returns the same lists: only the tiles that pass change.
constexpr int LSEED_MAX_SUB = 64;
constexpr int LSEED_SUB_DEFAULT = 32;
constexpr int LSEED_SUB_ITERS = 8;
constexpr int LSEED_SUB_MAX_DIM = 128;          // component slots of a packed cell: 32 per operand step, at most 4 steps

inline int lseed_sub_count(int option) { return option == 0 ? LSEED_SUB_DEFAULT : option < 1 ? 1 : option > LSEED_MAX_SUB ? LSEED_MAX_SUB : option; }
NABO_HD inline bool lseed_sub_applies(uint32_t ref_cnt, int S) { return S > 1 && ref_cnt >= (uint32_t)S; }
// which of a bucket's unmasked references (numbered in caller order) is sub-anchor j
NABO_HD inline uint32_t lseed_sub_anchor_cell(uint32_t ref_cnt, int S, int j) { return (uint32_t)j * (ref_cnt / (uint32_t)S); }
// the counting sort's key of a cell: (bucket, sub-rank)
NABO_HD inline uint32_t lseed_sub_key(int b, int S, int rank) { return (uint32_t)b * (uint32_t)S + (uint32_t)rank; }

// The ranking, element by element (the device runs one element per thread, the host loops): pts [S][dim] floats.
NABO_HD inline double lseed_sub_mean(int S, int dim, const float *pts, int d)
{
    double s = 0.0;
    for (int j = 0; j < S; ++j) s += (double)pts[j * dim + d];
    return s / S;
}
NABO_HD inline double lseed_sub_proj(int dim, const float *pt, const double *mean, const double *v)
{
    double s = 0.0;
    for (int d = 0; d < dim; ++d) s += ((double)pt[d] - mean[d]) * v[d];
    return s;
}
NABO_HD inline double lseed_sub_back(int S, int dim, const float *pts, const double *mean, const double *t, int d)
{
    double s = 0.0;
    for (int j = 0; j < S; ++j) s += t[j] * ((double)pts[j * dim + d] - mean[d]);
    return s;
}
NABO_HD inline double lseed_sub_sumsq(int dim, const double *w)
{
    double s = 0.0;
    for (int d = 0; d < dim; ++d) s += w[d] * w[d];
    return s;
}
// (a direction of length zero or not finite -- all sub-anchors equal, overflow -- is not taken: the one before it stays)
NABO_HD inline bool lseed_sub_dir_ok(double sumsq) { return sumsq > 0.0 && sumsq < 1.7976931348623157e308; }
NABO_HD inline int lseed_sub_rank_of(int S, const double *proj, int j)
{
    int r = 0;
    for (int i = 0; i < S; ++i) r += proj[i] < proj[j] || (proj[i] == proj[j] && i < j);
    return r;
}
// rank [S] of the sub-anchors pts [S][dim]; by_index: the plain rule, rank = j
inline void lseed_sub_ranks(int S, int dim, const float *pts, bool by_index, uint8_t *rank)
{
    double mean[LSEED_SUB_MAX_DIM], v[LSEED_SUB_MAX_DIM], w[LSEED_SUB_MAX_DIM], t[LSEED_MAX_SUB];
    for (int j = 0; j < S; ++j) rank[j] = (uint8_t)j;
    if (by_index || S > LSEED_MAX_SUB || dim > LSEED_SUB_MAX_DIM) return;
    for (int d = 0; d < dim; ++d) mean[d] = lseed_sub_mean(S, dim, pts, d);
    for (int d = 0; d < dim; ++d) v[d] = 1.0;
    for (int it = 0; it < LSEED_SUB_ITERS; ++it) {
        for (int j = 0; j < S; ++j) t[j] = lseed_sub_proj(dim, pts + j * dim, mean, v);
        for (int d = 0; d < dim; ++d) w[d] = lseed_sub_back(S, dim, pts, mean, t, d);
        const double ss = lseed_sub_sumsq(dim, w);
        if (!lseed_sub_dir_ok(ss)) break;
        const double inv = 1.0 / __builtin_sqrt(ss);
        for (int d = 0; d < dim; ++d) v[d] = w[d] * inv;
    }
    for (int j = 0; j < S; ++j) t[j] = lseed_sub_proj(dim, pts + j * dim, mean, v);
    for (int j = 0; j < S; ++j) rank[j] = (uint8_t)lseed_sub_rank_of(S, t, j);
}
// a cell's sub-anchor among a [S][dim] (norm [S] = ||a||^2): smallest norm - 2 a.v in fp32, ties to the lowest j
NABO_HD inline int lseed_sub_nearest(int S, int dim, const float *a, const float *norm, const float *v)
{
    float best = __builtin_inff();
    int bj = 0;
    for (int j = 0; j < S; ++j) {
        float d = 0.0f;
        for (int e = 0; e < dim; ++e) d = __builtin_fmaf(a[j * dim + e], v[e], d);
        const float sc = __builtin_fmaf(-2.0f, d, norm[j]);
        if (sc < best) { best = sc; bj = j; }
    }
    return bj;
}
// first position of every (bucket, rank) class: sub [C * S] from the buckets' first positions and the classes' sizes
NABO_HD inline void lseed_sub_layout(int b, int S, const int64_t *base, const uint32_t *subcnt, int64_t *sub)
{
    int64_t pos = base[b];
    for (int r = 0; r < S; ++r) {
        sub[(int64_t)b * S + r] = pos;
        pos += subcnt[(int64_t)b * S + r];
    }
}

// The whole rule on the host, for n cells [n][dim] with bucket[i] (-1: none, a masked reference) and the same cells as
// references and targets: pos[i] = position of cell i in the full ordered copy (lseed_layout_full), -1 for no bucket.
// S <= 1: the order by (bucket, caller order).  What tests/test_sub_order_cpu.py holds against its numpy restatement.
inline void lseed_sub_positions(int C, int S, int64_t n, int dim, const float *cells, const int32_t *bucket, bool by_index, int64_t *pos)
{
    uint32_t *cnt = new uint32_t[C]();
    int64_t *lay = new int64_t[3 * (C + 1)];
    for (int64_t i = 0; i < n; ++i)
        if (bucket[i] >= 0) ++cnt[bucket[i]];
    lseed_layout_full(C, cnt, lay, lay + (C + 1), lay + 2 * (C + 1));
    const int SS = S < 1 ? 1 : S;
    uint32_t *key = new uint32_t[n], *subcnt = new uint32_t[(int64_t)C * SS]();
    int64_t *sub = new int64_t[(int64_t)C * SS];
    float *a = new float[(int64_t)SS * dim], *norm = new float[SS];
    uint8_t *rank = new uint8_t[SS];
    for (int b = 0; b < C; ++b) {
        const bool on = lseed_sub_applies(cnt[b], SS);
        if (on) {
            uint32_t seen = 0;
            int j = 0;
            for (int64_t i = 0; i < n && j < SS; ++i) {
                if (bucket[i] != b) continue;
                if (seen++ != lseed_sub_anchor_cell(cnt[b], SS, j)) continue;
                for (int e = 0; e < dim; ++e) a[j * dim + e] = cells[i * dim + e];
                ++j;
            }
            for (j = 0; j < SS; ++j) {
                float s2 = 0.0f;
                for (int e = 0; e < dim; ++e) s2 = __builtin_fmaf(a[j * dim + e], a[j * dim + e], s2);
                norm[j] = s2;
            }
            lseed_sub_ranks(SS, dim, a, by_index, rank);
        }
        for (int64_t i = 0; i < n; ++i) {
            if (bucket[i] != b) continue;
            const int r = on ? rank[lseed_sub_nearest(SS, dim, a, norm, cells + i * dim)] : 0;
            key[i] = lseed_sub_key(b, SS, r);
            ++subcnt[key[i]];
        }
    }
    for (int b = 0; b < C; ++b) lseed_sub_layout(b, SS, lay, subcnt, sub);
    for (int64_t i = 0; i < n; ++i) pos[i] = bucket[i] >= 0 ? sub[key[i]]++ : -1;
    delete[] cnt; delete[] lay; delete[] key; delete[] subcnt; delete[] sub; delete[] a; delete[] norm; delete[] rank;
}

// The columns of class b (b == C: the rest class, whose tournament `rest` is the stream's own) get their range; columns
// no class reaches keep (0, 0, 0, 0) -- no tournament, nothing written.
NABO_HD inline void lseed_fill_columns(int b, int C, const uint32_t *ref_cnt, int cap, int lkeep, int tile0, LseedRange rest,
                                       const int64_t *base, const int64_t *pade, LseedRange *ranges, int64_t ncol)
{
    const LseedRange r = b < C ? lseed_bucket_range(b, ref_cnt[b], cap, lkeep, tile0) : rest;
    if (b < C && r.pt == 0) return;
    for (int64_t c = base[b] / LSEED_COL_ROWS; c < pade[b] / LSEED_COL_ROWS && c < ncol; ++c) ranges[c] = r;
}

// columns a query of `rows` rows can need: every class pads less than one column
inline int64_t lseed_columns(int64_t rows, int C) { return (rows + LSEED_COL_ROWS - 1) / LSEED_COL_ROWS + C + 1; }

}  // namespace nabo
