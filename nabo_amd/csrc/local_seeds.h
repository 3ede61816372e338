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
