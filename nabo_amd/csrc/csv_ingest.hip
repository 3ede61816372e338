// A dense CSV table of numbers -> its non-zero entries by row and by column, on the device (include/nabo_csv.h is the
// specification).
//
// The text arrives in pieces of whole fields (csv_host.h).  A FIELD belongs to the tile (CSV_TILE bytes) in which its first
// byte lies, and one workgroup owns one tile.  A field's row is the number of `\n` in front of it, its column the number of
// separators since the last `\n`, so three launches parse a piece:
//   csv_count_kernel   every tile publishes (newlines, separators behind its last newline);
//   csv_base_kernel    one workgroup scans the tiles with the segmented operator (a, b) -> (a.n + b.n, b.n ? b.s : a.s + b.s)
//                      from the piece's own base, which the host carries from piece to piece: every tile gets its (row, column);
//   csv_parse_kernel   loads the tile, 16 bytes in front of it and CSV_LOOK bytes of look-ahead into LDS with 16-byte loads,
//                      makes the `\n` and the separator-or-`\n` bit masks of every 16 bytes as it stores them, scans the lanes
//                      with the same operator, and lane l converts the fields that start in bytes [64 l, 64 l + 64) with
//                      csv_number.h -- the source the CPU tests check.
// At most 32 entries can start in 64 bytes (`1,1,1,...`), so lane l of tile t owns 32 slots of a staging area in device
// memory, fills the first of them in file order and publishes how many; csv_place_kernel scans the lanes' counts, takes the
// tile's base from a scan of the per-tile counts, and moves the entries to where they belong.  Nothing is ordered by an
// atomic: the one atomicMin (the lowest error) and the atomicAdds (the statistics) are integer and commute.  A field the
// device does not decide is staged like an entry with the top bit of its key set and its offset in the piece as its value;
// the place kernel lists such entries, the host converts them from the pinned text (csv_host.h) and a patch kernel stores
// the values; those that come to nothing are taken out by one compaction at finish.
// The text is read twice (count, parse), the second time out of the cache when a piece fits it; all writes are vector stores.
//
// finish: file order is (row, column) order, so key_rowptr_kernel gives row_ptr without a sort; the by-column index is
// mtx_transpose_stage (mtx_stages.h) with the entry's ordinal as the 4-byte payload and a gather of the 8-byte values.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/nabo_csv.h"
#include "csv_host.h"
#include "host_common.h"
#include "launch.h"
#include "mtx_stages.h"

namespace nabo {

constexpr int CSV_TILE = csv::TILE_BYTES, CSV_BLOCK = 256, CSV_LEAD = 16;
constexpr int CSV_LOOK = 1088;                                           // the longest field, its end, whole 64-byte mask words
constexpr int CSV_LANE_BYTES = CSV_TILE / CSV_BLOCK;                     // 64: one bit of a 64-bit mask per byte
constexpr int CSV_LANE_SLOTS = CSV_LANE_BYTES / 2;                       // 32: an entry has a byte and its separator at least
constexpr int CSV_TILE_SLOTS = CSV_BLOCK * CSV_LANE_SLOTS;
constexpr int CSV_LDS_PIECES = (CSV_LEAD + CSV_TILE + CSV_LOOK) / 16;
constexpr int CSV_SCAN_BLOCK = 1024;
constexpr uint64_t CSV_DEFERRED = (uint64_t)1 << 63;                     // in a staged key: the value is the field's offset
static_assert(CSV_LANE_BYTES == 64 && CSV_LOOK % 64 == 0 && CSV_LOOK > csv::MAX_FIELD && CSV_LOOK > csv::MAX_NAME, "one mask bit per byte, whole mask words");
static_assert(sizeof(uint4) * CSV_LDS_PIECES + 4 * (CSV_TILE + CSV_LOOK) / 16 + 64 <= 160 * 1024, "LDS of one workgroup");

struct CsvPieceResult {
    unsigned long long err;       // min over the errors of (byte offset in the piece << 8 | code); ~0: none
    unsigned long long nl_total;  // the `\n` of the piece
    unsigned long long col_end;   // the separators behind its last `\n` (the base included while there is none)
    unsigned long long fields, converted, deferred;
};

struct CsvParams {
    int64_t len, row0;
    uint32_t n_fields, has_names, name_cap;
    int32_t kind, has_thresh;
    double thresh;
    uint32_t sep4;                // the separator in every byte
};

struct NlSep {
    uint32_t n, s;                // newlines; separators behind the last of them
};
__device__ __forceinline__ NlSep csv_join(NlSep a, NlSep b) { return NlSep{a.n + b.n, b.n ? b.s : a.s + b.s}; }

// bit b (b < 4) is set when byte b of w equals the byte c4 repeats
__device__ __forceinline__ uint32_t csv_eq4(uint32_t w, uint32_t c4)
{
    const uint32_t x = w ^ c4;
    const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
    return ((z >> 7) * 0x01020408u) >> 24;
}
__device__ __forceinline__ uint32_t csv_eq16(uint4 p, uint32_t c4) { return csv_eq4(p.x, c4) | csv_eq4(p.y, c4) << 4 | csv_eq4(p.z, c4) << 8 | csv_eq4(p.w, c4) << 12; }
// the bits of a 16-byte piece at byte offset `at` that lie inside the text
__device__ __forceinline__ uint32_t csv_inside(int64_t at, int64_t len) { return len - at >= 16 ? 0xFFFFu : len - at <= 0 ? 0u : (1u << (len - at)) - 1u; }

// what a lane's 64 bytes add: their newlines and the separators behind the last of them
__device__ __forceinline__ NlSep csv_lane_sum(uint64_t ends, uint64_t nls)
{
    const uint64_t seps = ends & ~nls;
    const uint64_t above = nls ? ~(uint64_t)0 << (63 - __clzll((long long)nls)) : ~(uint64_t)0;   // from the last `\n` up (itself no separator)
    return NlSep{(uint32_t)__popcll(nls), (uint32_t)__popcll(seps & above)};
}

// exclusive prefix and total of the lanes' sums over the workgroup, in lane order
__device__ __forceinline__ void csv_block_scan(NlSep mine, NlSep *before, NlSep *total, NlSep *s_wave)
{
    const int ln = threadIdx.x & 63, w = threadIdx.x >> 6;
    NlSep inc = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        NlSep y;
        y.n = __shfl_up(inc.n, d, 64), y.s = __shfl_up(inc.s, d, 64);
        if (ln >= d) inc = csv_join(y, inc);
    }
    if (ln == 63) s_wave[w] = inc;
    __syncthreads();
    NlSep ex;
    ex.n = __shfl_up(inc.n, 1, 64), ex.s = __shfl_up(inc.s, 1, 64);
    if (ln == 0) ex = NlSep{0, 0};
    NlSep pre{0, 0}, tot{0, 0};
#pragma unroll
    for (int i = 0; i < CSV_BLOCK / 64; ++i) {
        if (i < w) pre = csv_join(pre, s_wave[i]);
        tot = csv_join(tot, s_wave[i]);
    }
    *before = csv_join(pre, ex);
    *total = tot;
}

__global__ __launch_bounds__(CSV_BLOCK) void csv_count_kernel(const uint4 *__restrict__ text, int64_t len, uint32_t sep4, uint2 *__restrict__ tile_sum)
{
    __shared__ NlSep s_wave[CSV_BLOCK / 64];
    const int64_t at = (int64_t)blockIdx.x * CSV_TILE + (int64_t)CSV_LANE_BYTES * threadIdx.x;
    uint64_t ends = 0, nls = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t a = at + 16 * k;
        if (a >= len) break;
        const uint4 p = text[a / 16];
        const uint32_t in = csv_inside(a, len), nl = csv_eq16(p, 0x0A0A0A0Au) & in, sp = csv_eq16(p, sep4) & in;
        nls |= (uint64_t)nl << (16 * k);
        ends |= (uint64_t)(nl | sp) << (16 * k);
    }
    NlSep before, total;
    csv_block_scan(csv_lane_sum(ends, nls), &before, &total, s_wave);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = make_uint2(total.n, total.s);
}

// one workgroup: base[t] = the join of (0, col0) and the sums of the tiles in front of t; the join of all of them to res
__global__ __launch_bounds__(CSV_SCAN_BLOCK) void csv_base_kernel(const uint2 *__restrict__ tile_sum, int64_t n_tiles, uint32_t col0, uint2 *__restrict__ base,
                                                                  CsvPieceResult *__restrict__ res)
{
    __shared__ NlSep s_part[CSV_SCAN_BLOCK];
    const int64_t per = (n_tiles + CSV_SCAN_BLOCK - 1) / CSV_SCAN_BLOCK, lo = std::min<int64_t>(per * threadIdx.x, n_tiles), hi = std::min<int64_t>(lo + per, n_tiles);
    NlSep acc{0, 0};
    for (int64_t t = lo; t < hi; ++t) acc = csv_join(acc, NlSep{tile_sum[t].x, tile_sum[t].y});
    s_part[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        NlSep run{0, col0};
        for (int i = 0; i < CSV_SCAN_BLOCK; ++i) {
            const NlSep mine = s_part[i];
            s_part[i] = run;
            run = csv_join(run, mine);
        }
        res->nl_total = run.n;
        res->col_end = run.s;
    }
    __syncthreads();
    NlSep run = s_part[threadIdx.x];
    for (int64_t t = lo; t < hi; ++t) {
        base[t] = make_uint2(run.n, run.s);
        run = csv_join(run, NlSep{tile_sum[t].x, tile_sum[t].y});
    }
}

// one workgroup: base[t] = the sum of cnt[0 .. t), t in [0, n_tiles]; both halves of the packed counts stay below 2^32
__global__ __launch_bounds__(CSV_SCAN_BLOCK) void csv_sum_kernel(const uint64_t *__restrict__ cnt, int64_t n_tiles, uint64_t *__restrict__ base)
{
    __shared__ uint64_t s_part[CSV_SCAN_BLOCK];
    const int64_t per = (n_tiles + CSV_SCAN_BLOCK - 1) / CSV_SCAN_BLOCK, lo = std::min<int64_t>(per * threadIdx.x, n_tiles), hi = std::min<int64_t>(lo + per, n_tiles);
    uint64_t acc = 0;
    for (int64_t t = lo; t < hi; ++t) acc += cnt[t];
    s_part[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t run = 0;
        for (int i = 0; i < CSV_SCAN_BLOCK; ++i) {
            const uint64_t mine = s_part[i];
            s_part[i] = run;
            run += mine;
        }
        base[n_tiles] = run;
    }
    __syncthreads();
    uint64_t run = s_part[threadIdx.x];
    for (int64_t t = lo; t < hi; ++t) {
        base[t] = run;
        run += cnt[t];
    }
}

// the bytes from tile offset p to the next separator or `\n`; limit + 1 when there is none within limit bytes
__device__ __forceinline__ int csv_field_len(const uint64_t *s_end, int p, int limit)
{
    int wi = p >> 6;
    const int b = p & 63;
    uint64_t m = s_end[wi] >> b;
    if (m) return min(__ffsll((unsigned long long)m) - 1, limit + 1);
    int n = 64 - b;
    while (n <= limit) {
        m = s_end[++wi];
        if (m) return min(n + __ffsll((unsigned long long)m) - 1, limit + 1);
        n += 64;
    }
    return limit + 1;
}

__global__ __launch_bounds__(CSV_BLOCK) void csv_parse_kernel(const uint4 *__restrict__ text, CsvParams P, const uint2 *__restrict__ base,
                                                              const uint64_t *__restrict__ pow5, uint4 *__restrict__ stage, uint16_t *__restrict__ lane_cnt,
                                                              uint64_t *__restrict__ tile_cnt, uint2 *__restrict__ name_pos, CsvPieceResult *__restrict__ res)
{
    __shared__ uint4 s_text[CSV_LDS_PIECES];
    __shared__ __attribute__((aligned(8))) uint16_t s_end[(CSV_TILE + CSV_LOOK) / 16];
    __shared__ __attribute__((aligned(8))) uint16_t s_nl[(CSV_TILE + CSV_LOOK) / 16];
    __shared__ NlSep s_wave[CSV_BLOCK / 64];
    __shared__ uint32_t s_cnt[2 * CSV_BLOCK / 64];
    const int tid = threadIdx.x;
    const int64_t len = P.len, tile0 = (int64_t)blockIdx.x * CSV_TILE;
    const int64_t n_pieces = (len + 15) / 16, piece0 = tile0 / 16 - 1;
    for (int k = tid; k < CSV_LDS_PIECES; k += CSV_BLOCK) {
        const int64_t gp = piece0 + k;
        uint4 p = make_uint4(0, 0, 0, 0);
        if (gp < 0) p.w = 0x0A000000u;                          // in front of the piece: a `\n`, so that byte 0 starts a field
        else if (gp < n_pieces) p = text[gp];
        s_text[k] = p;
        if (k >= 1) {
            const uint32_t in = csv_inside(gp * 16, len), nl = csv_eq16(p, 0x0A0A0A0Au) & in;
            s_nl[k - 1] = (uint16_t)nl;
            s_end[k - 1] = (uint16_t)(nl | (csv_eq16(p, P.sep4) & in));
        }
    }
    __syncthreads();
    const uint8_t *sb = reinterpret_cast<const uint8_t *>(s_text) + CSV_LEAD;      // byte 0 of the tile
    const uint64_t *end64 = reinterpret_cast<const uint64_t *>(s_end), *nl64 = reinterpret_cast<const uint64_t *>(s_nl);
    const uint64_t ends = end64[tid], nls = nl64[tid];
    NlSep before, total;
    csv_block_scan(csv_lane_sum(ends, nls), &before, &total, s_wave);
    const uint2 tb = base[blockIdx.x];
    uint32_t rowl = tb.x + before.n, col = before.n ? before.s : tb.y + before.s;   // of the lane's first byte, rows from the piece's start
    const int64_t left = len - (tile0 + (int64_t)CSV_LANE_BYTES * tid);
    const int sep = (int)(P.sep4 & 0xFF);
    uint4 *strip = stage + ((int64_t)blockIdx.x * CSV_BLOCK + tid) * CSV_LANE_SLOTS;
    uint32_t n_ent = 0, n_def = 0, n_fields = 0, n_conv = 0;
    unsigned long long err = ~0ull;
    auto fail = [&](int64_t at, int code) {
        const unsigned long long e = (unsigned long long)at << 8 | (unsigned)code;
        err = e < err ? e : err;
    };
    auto put = [&](uint64_t key, uint64_t val) {
        if (n_ent < CSV_LANE_SLOTS) strip[n_ent++] = make_uint4((uint32_t)key, (uint32_t)(key >> 32), (uint32_t)val, (uint32_t)(val >> 32));
    };
    // the field that starts at byte j of the lane, in column `col` of row `rowl`
    auto field = [&](int j) {
        if (col > P.n_fields) return;                           // behind the first field in excess
        const int p = CSV_LANE_BYTES * tid + j;
        const int64_t g = tile0 + p;
        if (col == P.n_fields) return fail(g, csv::ERR_TOO_MANY);
        const bool first = col == 0, is_name = first && P.has_names;
        const int limit = is_name ? csv::MAX_NAME : csv::MAX_FIELD;
        const int n = csv_field_len(end64, p, limit);
        const bool known = n <= limit, at_nl = known && (nl64[(p + n) >> 6] >> ((p + n) & 63) & 1);
        const uint8_t *s = sb + p;
        if (first && at_nl && (n == 0 || (n == 1 && s[0] == '\r'))) return fail(g, csv::ERR_EMPTY_LINE);
        if (is_name) {
            if (!known) fail(g, csv::ERR_NAME_LONG);
            else if (rowl < P.name_cap) name_pos[rowl] = make_uint2((uint32_t)g, (uint32_t)n);
        } else {
            ++n_fields;
            const uint64_t key = (uint64_t)(P.row0 + rowl) << 32 | (col - P.has_names);
            uint64_t bits = 0;
            const int code = known ? csv::convert_field(s, n, at_nl, P.kind, pow5, &bits) : (int)csv::DEFER;
            if (code == csv::VALUE) {
                ++n_conv;
                if (csv::keeps_value(P.kind, bits, P.has_thresh != 0, P.thresh)) put(key, bits);
            } else if (code == csv::DEFER) {
                ++n_def;
                put(key | CSV_DEFERRED, (uint64_t)g);
            } else
                fail(g, code);
        }
        if (at_nl && col + 1 < P.n_fields) fail(g + n, csv::ERR_TOO_FEW);
    };
    if (left > 0) {
        const uint8_t prev = sb[CSV_LANE_BYTES * tid - 1];
        if (prev == '\n' || prev == sep) field(0);
        uint64_t m = ends;
        while (m) {
            const int e = __ffsll((unsigned long long)m) - 1;
            m &= m - 1;
            if (nls >> e & 1) ++rowl, col = 0;
            else ++col;
            if (e + 1 < CSV_LANE_BYTES && e + 1 < left) field(e + 1);
        }
    }
    if (err != ~0ull) atomicMin(&res->err, err);
    lane_cnt[(int64_t)blockIdx.x * CSV_BLOCK + tid] = (uint16_t)(n_ent | n_def << 8);
    uint32_t a = n_ent | n_def << 16, b = n_fields | n_conv << 16;              // at most 8192 of each in a tile
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        a += __shfl_xor(a, d, 64);
        b += __shfl_xor(b, d, 64);
    }
    if ((tid & 63) == 0) s_cnt[2 * (tid >> 6)] = a, s_cnt[2 * (tid >> 6) + 1] = b;
    __syncthreads();
    if (tid == 0) {
        uint32_t ta = 0, tb2 = 0;
        for (int i = 0; i < CSV_BLOCK / 64; ++i) ta += s_cnt[2 * i], tb2 += s_cnt[2 * i + 1];
        tile_cnt[blockIdx.x] = (uint64_t)(ta & 0xFFFFu) | (uint64_t)(ta >> 16) << 32;
        atomicAdd(&res->fields, (unsigned long long)(tb2 & 0xFFFFu));
        atomicAdd(&res->converted, (unsigned long long)(tb2 >> 16));
        atomicAdd(&res->deferred, (unsigned long long)(ta >> 16));
    }
}

// the staged entries of tile blockIdx.x to out[done + ...] in file order; the deferred among them to def_list as
// (position behind `done`, offset of the field in the piece), in file order too
__global__ __launch_bounds__(CSV_BLOCK) void csv_place_kernel(const uint4 *__restrict__ stage, const uint16_t *__restrict__ lane_cnt,
                                                              const uint64_t *__restrict__ tile_base, int64_t done, int64_t cap, uint64_t *__restrict__ out_key,
                                                              uint64_t *__restrict__ out_val, uint2 *__restrict__ def_list, int64_t def_cap)
{
    __shared__ uint32_t s_wave[CSV_BLOCK / 64];
    const int tid = threadIdx.x, ln = tid & 63, w = tid >> 6;
    const uint32_t c = lane_cnt[(int64_t)blockIdx.x * CSV_BLOCK + tid], n_ent = c & 0xFFu, n_def = c >> 8;
    const uint32_t mine = n_ent | n_def << 16;
    uint32_t inc = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(inc, d, 64);
        if (ln >= d) inc += y;
    }
    if (ln == 63) s_wave[w] = inc;
    __syncthreads();
    uint32_t before = inc - mine;
#pragma unroll
    for (int i = 0; i < CSV_BLOCK / 64; ++i) before += i < w ? s_wave[i] : 0;
    const uint64_t tb = tile_base[blockIdx.x];
    const int64_t pos0 = (int64_t)(tb & 0xFFFFFFFFull) + (before & 0xFFFFu);
    int64_t d0 = (int64_t)(tb >> 32) + (before >> 16);
    const uint4 *strip = stage + ((int64_t)blockIdx.x * CSV_BLOCK + tid) * CSV_LANE_SLOTS;
    for (uint32_t i = 0; i < n_ent && i < (uint32_t)CSV_LANE_SLOTS; ++i) {
        const uint4 e = strip[i];
        const uint64_t key = (uint64_t)e.y << 32 | e.x, val = (uint64_t)e.w << 32 | e.z;
        const int64_t pos = pos0 + i;
        if (done + pos >= cap) continue;
        const bool deferred = (key & CSV_DEFERRED) != 0;
        out_key[done + pos] = key & ~CSV_DEFERRED;
        out_val[done + pos] = deferred ? 0 : val;
        if (deferred) {
            if (d0 < def_cap) def_list[d0] = make_uint2((uint32_t)pos, (uint32_t)val);
            ++d0;
        }
    }
}

__global__ __launch_bounds__(256) void csv_patch_kernel(const uint2 *__restrict__ def_list, const uint64_t *__restrict__ vals, int64_t n, int64_t done, int64_t cap,
                                                        uint64_t *__restrict__ out_val)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < n && done + def_list[k].x < cap) out_val[done + def_list[k].x] = vals[k];
}

// entry i moves down by the number of dropped entries in front of it; drop [n_drop] ascending
__global__ __launch_bounds__(256) void csv_compact_kernel(const uint64_t *__restrict__ key, const uint64_t *__restrict__ val, int64_t n, const int64_t *__restrict__ drop,
                                                          int64_t n_drop, uint64_t *__restrict__ out_key, uint64_t *__restrict__ out_val)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int64_t lo = 0, hi = n_drop;                                // the first dropped entry at or behind i
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (drop[mid] < i) lo = mid + 1;
        else hi = mid;
    }
    if (lo < n_drop && drop[lo] == i) return;
    out_key[i - lo] = key[i];
    out_val[i - lo] = val[i];
}

__global__ __launch_bounds__(256) void csv_iota_kernel(uint32_t *__restrict__ out, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (uint32_t)i;
}

__global__ __launch_bounds__(256) void csv_gather_kernel(const uint64_t *__restrict__ val, const uint32_t *__restrict__ ord, int64_t n, uint64_t *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = val[ord[i]];
}

static unsigned csv_grid(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace nabo

// ---- the C ABI --------------------------------------------------------------------------------------------------------
using nabo::DevBuf;
namespace csv = nabo::csv;

struct nabo_csv {
    int device = 0;
    int64_t budget = 0, first_line = 0;
    uint8_t sep = ',';
    int64_t n_cols = 0;
    int has_names = 0, kind = 0, has_thresh = 0;
    double thresh = 0;
    csv::FieldBuffer fields;
    uint8_t *pinned = nullptr;
    bool finished = false, failed = false;
    int64_t rows_done = 0, col_carry = 0, entries_done = 0, cap = 0, n_chunks = 0, nnz = 0;
    int64_t pending_empty = 0;                                  // empty lines at the end of what has been parsed so far
    int64_t n_tiles_cap = 0, name_cap = 0, def_cap = 0, fixed_bytes = 0;
    int64_t stats[4] = {0, 0, 0, 0};
    double ms[4] = {0, 0, 0, 0};
    std::vector<int64_t> drops, name_off;
    std::string names;
    std::vector<uint2> h_def;
    std::vector<uint64_t> h_val;
    std::vector<uint2> h_name;
    nabo::Events<4> ev;
    DevBuf d_text, d_sum, d_base, d_stage, d_lane, d_cnt, d_cbase, d_name, d_def, d_defval, d_pow5, d_res;
    DevBuf d_key[2], d_ord[2], d_val, d_colval, d_col, d_row_ptr, d_col_ptr, d_temp, d_drop;
    int which = 0;
    uint32_t *d_rows = nullptr;
    ~nabo_csv()
    {
        if (pinned) (void)hipHostFree(pinned);
    }
};

namespace {

const uint64_t *pow5_table()
{
    static const std::vector<uint64_t> table = [] {
        std::vector<uint64_t> t((size_t)csv::POW5_WORDS);
        csv::build_pow5(t.data());
        return t;
    }();
    return table.data();
}

int csv_fail(nabo_csv *h, int rc)
{
    h->failed = true;
    return rc;
}

int csv_error_at(nabo_csv *h, int64_t line, int64_t field, int code)
{
    return nabo::api_fail(NABO_E_INVALID, "line %lld, field %lld: %s", (long long)(h->first_line + line), (long long)field, csv::code_text(code));
}

// the error (offset << 8 | code) of the piece in the pinned buffer
int csv_piece_error(nabo_csv *h, unsigned long long err)
{
    const int code = (int)(err & 0xFF);
    const csv::Place p = csv::locate(h->fields.buf, (int64_t)(err >> 8), h->sep, h->col_carry);
    return csv_error_at(h, h->rows_done + p.line + 1, p.field + (code == csv::ERR_TOO_FEW ? 2 : 1), code);
}

// the bytes per entry of the finished handle: two key buffers, two ordinal buffers, the values twice, the columns
constexpr int64_t ENTRY_BYTES = 16 + 8 + 16 + 4;

// room for `need` entries: doubling while the budget allows it, `need` exactly when it does not
int csv_grow(nabo_csv *h, int64_t need)
{
    if (need <= h->cap) return NABO_OK;
    if (need >= 0xFFFFFFFFll) return nabo::api_fail(NABO_E_UNSUPPORTED, "the table has %lld entries or more; nnz must be below 2^32 - 1", (long long)need);
    int64_t want = std::max<int64_t>(std::max<int64_t>(2 * h->cap, need), 1 << 16);
    if (h->fixed_bytes + ENTRY_BYTES * want > h->budget) want = need;
    if (h->fixed_bytes + ENTRY_BYTES * want > h->budget)
        return nabo::api_fail(NABO_E_NOMEM, "%lld entries with chunks of %lld bytes need %lld bytes of device memory, the budget is %lld", (long long)need,
                              (long long)h->fields.chunk, (long long)(h->fixed_bytes + ENTRY_BYTES * want), (long long)h->budget);
    DevBuf key, val;
    HIP_TRY(key.alloc((size_t)want * 8));
    HIP_TRY(val.alloc((size_t)want * 8));
    if (h->entries_done > 0) {
        HIP_TRY(hipMemcpyAsync(key.p, h->d_key[0].p, (size_t)h->entries_done * 8, hipMemcpyDeviceToDevice, nullptr));
        HIP_TRY(hipMemcpyAsync(val.p, h->d_val.p, (size_t)h->entries_done * 8, hipMemcpyDeviceToDevice, nullptr));
        HIP_TRY(hipStreamSynchronize(nullptr));
    }
    std::swap(h->d_key[0].p, key.p), std::swap(h->d_key[0].cap, key.cap);
    std::swap(h->d_val.p, val.p), std::swap(h->d_val.cap, val.cap);
    h->cap = want;
    return NABO_OK;
}

// upload and parse fields.buf[0, len): whole fields, the last byte a separator or a `\n`
int csv_parse_piece(nabo_csv *h, int64_t len)
{
    if (len <= 0) return NABO_OK;
    const uint8_t *buf = h->fields.buf;
    if (h->pending_empty > 0) {
        // empty lines were the end of the table so far: they stay that only if nothing else follows
        if (!csv::only_empty_lines(buf, 0, len)) return csv_error_at(h, h->rows_done + 1, 1, csv::ERR_EMPTY_LINE);
        h->pending_empty += (int64_t)std::count(buf, buf + len, (uint8_t)'\n');
        return NABO_OK;
    }
    hipStream_t st = nullptr;
    const int64_t padded = (len + 15) / 16 * 16, n_tiles = (len + csv::TILE_BYTES - 1) / csv::TILE_BYTES;
    nabo::CsvPieceResult res;
    nabo::CsvPieceResult *d_res = h->d_res.as<nabo::CsvPieceResult>();
    nabo::CsvParams P;
    P.len = len, P.row0 = h->rows_done, P.n_fields = (uint32_t)(h->n_cols + h->has_names), P.has_names = (uint32_t)h->has_names;
    P.name_cap = (uint32_t)h->name_cap, P.kind = h->kind, P.has_thresh = h->has_thresh, P.thresh = h->thresh, P.sep4 = 0x01010101u * h->sep;
    uint64_t total = 0;
    HIP_TRY(hipEventRecord(h->ev.ev[0], st));
    HIP_TRY(hipMemcpyAsync(h->d_text.p, buf, (size_t)len, hipMemcpyHostToDevice, st));
    if (padded > len) HIP_TRY(hipMemsetAsync(h->d_text.as<uint8_t>() + len, 0, (size_t)(padded - len), st));
    HIP_TRY(hipEventRecord(h->ev.ev[1], st));
    HIP_TRY(hipMemsetAsync(d_res, 0, sizeof res, st));
    HIP_TRY(hipMemsetAsync(d_res, 0xFF, sizeof(unsigned long long), st));
    if (h->has_names) HIP_TRY(hipMemsetAsync(h->d_name.p, 0xFF, (size_t)h->name_cap * 8, st));
    hipLaunchKernelGGL(nabo::csv_count_kernel, dim3((unsigned)n_tiles), dim3(nabo::CSV_BLOCK), 0, st, h->d_text.as<uint4>(), len, P.sep4, h->d_sum.as<uint2>());
    hipLaunchKernelGGL(nabo::csv_base_kernel, dim3(1), dim3(nabo::CSV_SCAN_BLOCK), 0, st, h->d_sum.as<uint2>(), n_tiles, (uint32_t)h->col_carry,
                       h->d_base.as<uint2>(), d_res);
    hipLaunchKernelGGL(nabo::csv_parse_kernel, dim3((unsigned)n_tiles), dim3(nabo::CSV_BLOCK), 0, st, h->d_text.as<uint4>(), P, h->d_base.as<uint2>(),
                       h->d_pow5.as<uint64_t>(), h->d_stage.as<uint4>(), h->d_lane.as<uint16_t>(), h->d_cnt.as<uint64_t>(), h->d_name.as<uint2>(), d_res);
    hipLaunchKernelGGL(nabo::csv_sum_kernel, dim3(1), dim3(nabo::CSV_SCAN_BLOCK), 0, st, h->d_cnt.as<uint64_t>(), n_tiles, h->d_cbase.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&res, d_res, sizeof res, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&total, h->d_cbase.as<uint64_t>() + n_tiles, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t n_ent = (int64_t)(total & 0xFFFFFFFFull), n_def = (int64_t)(total >> 32);
    if (n_def > h->def_cap) return nabo::api_fail(NABO_E_HIP, "%lld deferred fields in a piece that can hold %lld", (long long)n_def, (long long)h->def_cap);
    int rc = csv_grow(h, h->entries_done + n_ent);
    if (rc) return rc;
    if (n_ent > 0) {
        hipLaunchKernelGGL(nabo::csv_place_kernel, dim3((unsigned)n_tiles), dim3(nabo::CSV_BLOCK), 0, st, h->d_stage.as<uint4>(), h->d_lane.as<uint16_t>(),
                           h->d_cbase.as<uint64_t>(), h->entries_done, h->cap, h->d_key[0].as<uint64_t>(), h->d_val.as<uint64_t>(), h->d_def.as<uint2>(),
                           h->def_cap);
        HIP_TRY(hipGetLastError());
    }
    unsigned long long err = res.err;
    if (n_def > 0) {
        // the fields the device left to the host, from the text that is still here
        h->h_def.resize((size_t)n_def);
        h->h_val.resize((size_t)n_def);
        HIP_TRY(hipMemcpyAsync(h->h_def.data(), h->d_def.p, (size_t)n_def * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (int64_t k = 0; k < n_def; ++k) {
            const int64_t at = h->h_def[(size_t)k].y, n = csv::field_length(buf, at, len, h->sep);
            const bool at_nl = buf[at + n] == '\n';
            uint64_t bits = 0;
            const int code = csv::host_convert(buf + at, n, at_nl, h->kind, &bits);
            if (code) err = std::min(err, (unsigned long long)at << 8 | (unsigned)code);
            // the device judges the end of a line where it sees it: not behind a field longer than max_field
            if (n > csv::MAX_FIELD && at_nl && csv::locate(buf, at, h->sep, h->col_carry).field + 1 < h->n_cols + h->has_names)
                err = std::min(err, (unsigned long long)(at + n) << 8 | (unsigned)csv::ERR_TOO_FEW);
            h->h_val[(size_t)k] = bits;
            if (code || !csv::keeps_value(h->kind, bits, h->has_thresh != 0, h->thresh)) h->drops.push_back(h->entries_done + h->h_def[(size_t)k].x);
        }
        HIP_TRY(hipMemcpyAsync(h->d_defval.p, h->h_val.data(), (size_t)n_def * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(nabo::csv_patch_kernel, dim3(nabo::csv_grid(n_def)), dim3(256), 0, st, h->d_def.as<uint2>(), h->d_defval.as<uint64_t>(), n_def,
                           h->entries_done, h->cap, h->d_val.as<uint64_t>());
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(h->ev.ev[2], st));
    int64_t empties = 0;
    if (err != ~0ull) {
        const int64_t at = (int64_t)(err >> 8);
        if ((int)(err & 0xFF) != csv::ERR_EMPTY_LINE || !csv::only_empty_lines(buf, at, len)) return csv_piece_error(h, err);
        empties = (int64_t)std::count(buf + at, buf + len, (uint8_t)'\n');
    }
    const int64_t n_lines = (int64_t)res.nl_total - empties;
    if (h->rows_done + n_lines >= ((int64_t)1 << 31) - 1) return nabo::api_fail(NABO_E_UNSUPPORTED, "the table must have fewer than 2^31 - 1 rows");
    if (h->has_names) {
        // the first field of every line that starts in this piece, from the pinned text
        const int64_t slots = std::min<int64_t>((int64_t)res.nl_total + 1, h->name_cap);
        h->h_name.resize((size_t)slots);
        HIP_TRY(hipMemcpyAsync(h->h_name.data(), h->d_name.p, (size_t)slots * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (int64_t k = 0; k < slots; ++k) {
            const uint2 np = h->h_name[(size_t)k];
            if (np.x == 0xFFFFFFFFu) continue;
            h->names.append(reinterpret_cast<const char *>(buf) + np.x, (size_t)np.y);
            h->name_off.push_back((int64_t)h->names.size());
        }
    }
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(h->ev.elapsed(0, 1, &h->ms[0]));
    HIP_TRY(h->ev.elapsed(1, 2, &h->ms[1]));
    ++h->n_chunks;
    h->rows_done += n_lines;
    h->pending_empty = empties;
    h->col_carry = (int64_t)res.col_end;
    h->entries_done += n_ent;
    h->stats[0] += (int64_t)res.fields, h->stats[2] += (int64_t)res.converted, h->stats[3] += (int64_t)res.deferred;
    return NABO_OK;
}

int csv_feed_bytes(nabo_csv *h, const uint8_t *p, int64_t n)
{
    while (n > 0) {
        const int64_t took = h->fields.push(p, n);
        p += took, n -= took;
        if (!h->fields.ready()) continue;
        const int64_t len = h->fields.piece();
        if (len == 0) {
            if (h->fields.too_long()) {
                if (h->pending_empty > 0) return csv_error_at(h, h->rows_done + 1, 1, csv::ERR_EMPTY_LINE);
                const csv::Place at = csv::locate(h->fields.buf, 0, h->sep, h->col_carry);
                return csv_error_at(h, h->rows_done + 1, at.field + 1, csv::ERR_FIELD_LONG);
            }
            continue;
        }
        const int rc = csv_parse_piece(h, len);
        if (rc) return rc;
        h->fields.drop(len);
    }
    return NABO_OK;
}

int csv_check_handle(nabo_csv *h, bool want_finished)
{
    if (!h) return nabo::api_fail(NABO_E_INVALID, "the reader is NULL");
    if (h->failed) return nabo::api_fail(NABO_E_INVALID, "the reader has failed before; only nabo_csv_free is left");
    if (want_finished != h->finished)
        return nabo::api_fail(NABO_E_INVALID, want_finished ? "nabo_csv_finish has not been called" : "nabo_csv_finish has been called already");
    return NABO_OK;
}

int csv_download(nabo_csv *h, void *dst, const void *src, size_t bytes)
{
    if (!dst || !bytes) return NABO_OK;
    HIP_TRY(hipEventRecord(h->ev.ev[0], nullptr));
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipEventRecord(h->ev.ev[1], nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(h->ev.elapsed(0, 1, &h->ms[3]));
    return NABO_OK;
}

// every buffer a piece needs; what they come to is fixed_bytes
int csv_allocate(nabo_csv *h)
{
    const int64_t max_piece = h->fields.max_piece(), t = (max_piece + csv::TILE_BYTES - 1) / csv::TILE_BYTES;
    h->n_tiles_cap = t;
    h->name_cap = h->has_names ? max_piece / (2 * (h->n_cols + 1)) + 2 : 0;        // a line with a name has 2 (n_cols + 1) bytes at least
    h->def_cap = max_piece / 5 + 2;                                                // a deferred field has 4 bytes and its end at least
    h->fixed_bytes = (max_piece + 16) + t * ((int64_t)nabo::CSV_TILE_SLOTS * 16 + nabo::CSV_BLOCK * 2 + 32) + 8 * h->name_cap + 16 * h->def_cap
                     + 8 * csv::POW5_WORDS + 8 * (h->n_cols + 1) + 256;
    if (h->fixed_bytes > h->budget)
        return nabo::api_fail(NABO_E_NOMEM, "chunks of %lld bytes need %lld bytes of device memory before the first entry, the budget is %lld",
                              (long long)h->fields.chunk, (long long)h->fixed_bytes, (long long)h->budget);
    HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&h->pinned), (size_t)max_piece, hipHostMallocDefault));
    h->fields.buf = h->pinned;
    HIP_TRY(h->d_text.alloc((size_t)((max_piece + 15) / 16 * 16)));
    HIP_TRY(h->d_sum.alloc((size_t)t * 8));
    HIP_TRY(h->d_base.alloc((size_t)t * 8));
    HIP_TRY(h->d_stage.alloc((size_t)t * nabo::CSV_TILE_SLOTS * 16));
    HIP_TRY(h->d_lane.alloc((size_t)t * nabo::CSV_BLOCK * 2));
    HIP_TRY(h->d_cnt.alloc((size_t)t * 8));
    HIP_TRY(h->d_cbase.alloc((size_t)(t + 1) * 8));
    HIP_TRY(h->d_name.alloc((size_t)h->name_cap * 8));
    HIP_TRY(h->d_def.alloc((size_t)h->def_cap * 8));
    HIP_TRY(h->d_defval.alloc((size_t)h->def_cap * 8));
    HIP_TRY(h->d_pow5.alloc((size_t)csv::POW5_WORDS * 8));
    HIP_TRY(h->d_res.alloc(sizeof(nabo::CsvPieceResult)));
    HIP_TRY(hipMemcpy(h->d_pow5.p, pow5_table(), (size_t)csv::POW5_WORDS * 8, hipMemcpyHostToDevice));
    HIP_TRY(h->ev.create());
    h->name_off.push_back(0);
    return NABO_OK;
}

// row_ptr, the columns, and the by-column index of the nnz entries in d_key[which] / d_val
int csv_index(nabo_csv *h, int64_t n_rows)
{
    hipStream_t st = nullptr;
    const int64_t n0 = h->entries_done, n_drop = (int64_t)h->drops.size(), nnz = n0 - n_drop;
    size_t sort = 0;
    HIP_TRY(nabo::mtx_sort_temp_bytes(nnz, n_rows, h->n_cols, &sort));
    const int64_t peak = h->fixed_bytes + ENTRY_BYTES * std::max<int64_t>(h->cap, n0) + 8 * (n_rows + 1) + (int64_t)sort + 8 * n_drop;
    if (peak > h->budget)
        return nabo::api_fail(NABO_E_NOMEM, "%lld entries in %lld rows need %lld bytes of device memory, the budget is %lld", (long long)nnz, (long long)n_rows,
                              (long long)peak, (long long)h->budget);
    if (h->cap == 0) {
        HIP_TRY(h->d_key[0].alloc(8));
        HIP_TRY(h->d_val.alloc(8));
    }
    HIP_TRY(h->d_key[1].alloc((size_t)n0 * 8));
    HIP_TRY(h->d_colval.alloc((size_t)n0 * 8));
    HIP_TRY(h->d_ord[0].alloc((size_t)nnz * 4));
    HIP_TRY(h->d_ord[1].alloc((size_t)nnz * 4));
    HIP_TRY(h->d_col.alloc((size_t)nnz * 4));
    HIP_TRY(h->d_row_ptr.alloc((size_t)(n_rows + 1) * 8));
    HIP_TRY(h->d_col_ptr.alloc((size_t)(h->n_cols + 1) * 8));
    HIP_TRY(h->d_temp.alloc(sort));
    HIP_TRY(hipEventRecord(h->ev.ev[0], st));
    h->which = 0;
    if (n_drop > 0) {
        // deferred fields that came to nothing: every entry behind one moves down
        std::sort(h->drops.begin(), h->drops.end());
        HIP_TRY(h->d_drop.alloc((size_t)n_drop * 8));
        HIP_TRY(hipMemcpyAsync(h->d_drop.p, h->drops.data(), (size_t)n_drop * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(nabo::csv_compact_kernel, dim3(nabo::csv_grid(n0)), dim3(256), 0, st, h->d_key[0].as<uint64_t>(), h->d_val.as<uint64_t>(), n0,
                           h->d_drop.as<int64_t>(), n_drop, h->d_key[1].as<uint64_t>(), h->d_colval.as<uint64_t>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
        std::swap(h->d_val.p, h->d_colval.p), std::swap(h->d_val.cap, h->d_colval.cap);
        h->which = 1;
    }
    uint64_t *keys = h->d_key[h->which].as<uint64_t>();
    if (nnz > 0) {
        HIP_TRY(nabo::key_rowptr_launch(keys, nnz, n_rows, h->d_row_ptr.as<int64_t>(), st));
        HIP_TRY(nabo::mtx_split_launch(keys, nnz, h->d_col.as<uint32_t>(), nullptr, st));
        hipLaunchKernelGGL(nabo::csv_iota_kernel, dim3(nabo::csv_grid(nnz)), dim3(256), 0, st, h->d_ord[h->which].as<uint32_t>(), nnz);
        HIP_TRY(hipGetLastError());
    } else
        HIP_TRY(hipMemsetAsync(h->d_row_ptr.p, 0, (size_t)(n_rows + 1) * 8, st));
    const int rc = nabo::mtx_transpose_stage(h->d_key, h->d_ord, &h->which, nnz, n_rows, h->n_cols, h->d_temp.p, h->d_temp.cap, h->d_col_ptr.as<int64_t>(),
                                             &h->d_rows, st);
    if (rc) return rc;
    if (nnz > 0) {
        hipLaunchKernelGGL(nabo::csv_gather_kernel, dim3(nabo::csv_grid(nnz)), dim3(256), 0, st, h->d_val.as<uint64_t>(), h->d_ord[h->which].as<uint32_t>(), nnz,
                           h->d_colval.as<uint64_t>());
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(h->ev.ev[1], st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(h->ev.elapsed(0, 1, &h->ms[2]));
    h->nnz = nnz;
    h->stats[1] = nnz;
    return NABO_OK;
}

}  // namespace

extern "C" {

int nabo_csv_create(int32_t device, int32_t sep, int64_t n_cols, int32_t has_row_names, int32_t value_kind, int32_t has_null_thresh, double null_thresh,
                    int64_t chunk_bytes, int64_t mem_budget_bytes, nabo_csv **out)
{
    if (!out) return nabo::api_fail(NABO_E_INVALID, "out is NULL");
    *out = nullptr;
    if (sep < 0 || sep > 255 || sep == '\n' || sep == '\r' || (sep >= '0' && sep <= '9'))
        return nabo::api_fail(NABO_E_INVALID, "sep=%d must be one byte, and not a line end or a digit", (int)sep);
    if (n_cols < 1 || n_cols >= ((int64_t)1 << 31) - 1) return nabo::api_fail(NABO_E_INVALID, "n_cols=%lld out of range [1, 2^31 - 1)", (long long)n_cols);
    if (value_kind != csv::KIND_FLOAT64 && value_kind != csv::KIND_INT64) return nabo::api_fail(NABO_E_INVALID, "value_kind=%d must be 0 (float64) or 1 (int64)", (int)value_kind);
    if (has_null_thresh && null_thresh != null_thresh) return nabo::api_fail(NABO_E_INVALID, "null_thresh is not a number");
    int rc = nabo::use_device(device);
    if (rc) return rc;
    return nabo::create_handle(out, device, "nabo_csv_create", [&](nabo_csv *h) {
        h->sep = (uint8_t)sep, h->n_cols = n_cols, h->has_names = has_row_names != 0, h->kind = value_kind;
        h->has_thresh = has_null_thresh != 0, h->thresh = has_null_thresh ? null_thresh : 0.0;
        h->fields.sep = (uint8_t)sep;
        h->fields.chunk = csv::FieldBuffer::clamp_chunk(chunk_bytes);
        h->budget = mem_budget_bytes;
        if (mem_budget_bytes <= 0) {
            size_t free_b = 0, total_b = 0;
            HIP_TRY(hipMemGetInfo(&free_b, &total_b));
            h->budget = (int64_t)(free_b / 4 * 3);
        }
        return csv_allocate(h);
    });
}

int nabo_csv_set_first_line(nabo_csv *h, int64_t first_line)
{
    const int rc = csv_check_handle(h, false);
    if (rc) return rc;
    if (first_line < 0) return nabo::api_fail(NABO_E_INVALID, "first_line is negative");
    h->first_line = first_line;
    return NABO_OK;
}

int nabo_csv_feed(nabo_csv *h, const void *bytes, int64_t n)
{
    int rc = csv_check_handle(h, false);
    if (rc) return rc;
    if (n < 0 || (n > 0 && !bytes)) return nabo::api_fail(NABO_E_INVALID, "bytes is NULL or n negative");
    if ((rc = nabo::use_device(h->device))) return csv_fail(h, rc);
    try {
        if ((rc = csv_feed_bytes(h, static_cast<const uint8_t *>(bytes), n))) return csv_fail(h, rc);
    } catch (const std::bad_alloc &) {
        return csv_fail(h, nabo::api_fail(NABO_E_NOMEM, "nabo_csv_feed: out of host memory"));
    }
    return NABO_OK;
}

int nabo_csv_finish(nabo_csv *h, int64_t *n_rows, int64_t *nnz)
{
    int rc = csv_check_handle(h, false);
    if (rc) return rc;
    if ((rc = nabo::use_device(h->device))) return csv_fail(h, rc);
    try {
        if ((rc = csv_parse_piece(h, h->fields.close()))) return csv_fail(h, rc);
        h->fields.size = 0;
        if ((rc = csv_index(h, h->rows_done))) return csv_fail(h, rc);
    } catch (const std::bad_alloc &) {
        return csv_fail(h, nabo::api_fail(NABO_E_NOMEM, "nabo_csv_finish: out of host memory"));
    }
    h->finished = true;
    if (n_rows) *n_rows = h->rows_done;
    if (nnz) *nnz = h->nnz;
    return NABO_OK;
}

int nabo_csv_get_rows(nabo_csv *h, int64_t *row_ptr, int32_t *col, void *val)
{
    int rc = csv_check_handle(h, true);
    if (rc || (rc = nabo::use_device(h->device))) return rc;
    if ((rc = csv_download(h, row_ptr, h->d_row_ptr.p, (size_t)(h->rows_done + 1) * 8))) return rc;
    if ((rc = csv_download(h, col, h->d_col.p, (size_t)h->nnz * 4))) return rc;
    return csv_download(h, val, h->d_val.p, (size_t)h->nnz * 8);
}

int nabo_csv_get_cols(nabo_csv *h, int64_t *col_ptr, int32_t *row, void *val)
{
    int rc = csv_check_handle(h, true);
    if (rc || (rc = nabo::use_device(h->device))) return rc;
    if ((rc = csv_download(h, col_ptr, h->d_col_ptr.p, (size_t)(h->n_cols + 1) * 8))) return rc;
    if ((rc = csv_download(h, row, h->d_rows, (size_t)h->nnz * 4))) return rc;
    return csv_download(h, val, h->d_colval.p, (size_t)h->nnz * 8);
}

int nabo_csv_get_row_names(nabo_csv *h, int64_t *name_off, void *name_bytes)
{
    const int rc = csv_check_handle(h, true);
    if (rc) return rc;
    if (!h->has_names) return nabo::api_fail(NABO_E_INVALID, "the reader was created without row names");
    if (name_off) memcpy(name_off, h->name_off.data(), h->name_off.size() * 8);
    if (name_bytes && !h->names.empty()) memcpy(name_bytes, h->names.data(), h->names.size());
    return NABO_OK;
}

int nabo_csv_stats(nabo_csv *h, int64_t out[4])
{
    if (!h || !out) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    for (int i = 0; i < 4; ++i) out[i] = h->stats[i];
    if (!h->finished) out[1] = h->entries_done - (int64_t)h->drops.size();
    return NABO_OK;
}

int nabo_csv_last_device_ms(nabo_csv *h, double ms[4], int64_t *n_chunks)
{
    if (!h || !ms) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    for (int i = 0; i < 4; ++i) ms[i] = h->ms[i];
    if (n_chunks) *n_chunks = h->n_chunks;
    return NABO_OK;
}

int nabo_csv_geometry(int32_t *tile_bytes, int32_t *max_field, int32_t *max_name)
{
    if (!tile_bytes || !max_field || !max_name) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    *tile_bytes = csv::TILE_BYTES;
    *max_field = csv::MAX_FIELD;
    *max_name = csv::MAX_NAME;
    return NABO_OK;
}

void nabo_csv_free(nabo_csv *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    delete h;
}

}  // extern "C"
