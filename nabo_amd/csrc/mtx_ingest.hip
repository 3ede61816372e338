// Matrix Market counts -> CSR by cell and CSC by gene, on the device (include/nabo_ingest.h is the specification).
//
// The text arrives in pieces of whole lines (mtx_host.h).  A line belongs to the tile (MTX_TILE bytes) in which its first
// byte lies and one workgroup owns one tile: it loads the tile, 16 bytes in front of it and MTX_ML bytes of look-ahead into
// LDS with 16-byte loads, makes the `\n` bit mask of every 16 bytes as it stores them, and lane l parses the lines that
// start in bytes [64 l, 64 l + 64) of the tile, byte by byte from LDS.  At most 11 entry lines can start in 64 bytes (the
// shortest is `1 1 1\n`), so a lane keeps its entries in 11 LDS slots of its own until the workgroup scan of the entry
// counts has given it its place in the tile; the tile's entries go to a staging area in file order, a rocPRIM exclusive scan
// of the per-tile counts gives every tile its base, and mtx_place_kernel moves the staged entries to where they belong.
// Nothing is ordered by an atomic: the one atomicMin (the lowest bad line) and the one atomicAdd (the number of lines, per
// workgroup) are integer and commute.  The text is read once from HBM; all writes are vector stores.
//
// finish: radix sort of (cell << 32 | gene, value) over the gene's bits and then the cell's bits (rocPRIM's LSD sort is
// stable, so the two calls are one sort over the bits in use), equal neighbours are duplicates, key_rowptr_kernel gives
// cell_ptr; a stable sort over the gene's bits alone then gives the (gene, cell) order, and csr_rowptr_kernel gene_ptr.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "../../include/nabo_ingest.h"
#include "host_common.h"
#include "launch.h"
#include "mtx_host.h"
#include "mtx_stages.h"

namespace nabo {

constexpr int MTX_TILE = mtx::TILE_BYTES, MTX_ML = mtx::MAX_LINE, MTX_BLOCK = 256, MTX_LEAD = 16;
constexpr int MTX_LANE_BYTES = MTX_TILE / MTX_BLOCK;                     // 64: one bit of a 64-bit mask per byte
constexpr int MTX_LANE_ENTRIES = (MTX_LANE_BYTES + 5) / 6;               // 11
constexpr int MTX_TILE_ENTRIES = MTX_TILE / 6 + 2;                       // entry lines are 6 bytes apart at least
constexpr int MTX_LDS_PIECES = (MTX_LEAD + MTX_TILE + MTX_ML) / 16;
static_assert(MTX_LANE_BYTES == 64 && MTX_ML % 16 == 0 && MTX_TILE % 16 == 0, "one mask bit per byte, whole 16-byte pieces");

int mtx_tile_entries() { return MTX_TILE_ENTRIES; }

// bit b (b < 4) is set when byte b of w is `\n`
__device__ __forceinline__ uint32_t mtx_nl4(uint32_t w)
{
    const uint32_t x = w ^ 0x0A0A0A0Au;
    const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);   // 0x80 in every byte of x that is zero
    return ((z >> 7) * 0x01020408u) >> 24;                                         // bits 0, 8, 16, 24 -> 24 .. 27, no carries
}

// The line that starts at s (LDS): mtx::parse_line (mtx_host.h) without a known length.  s may be read up to s[MTX_ML].
__device__ __forceinline__ int mtx_parse_line(const uint8_t *s, int64_t n_genes, int64_t n_cells, uint64_t *key, uint32_t *val)
{
    uint64_t f0 = 0, f1 = 0, f2 = 0, v = 0;
    int nf = 0, nd = 0, bad = 0;
    unsigned over = 0;
    bool indig = false, seen = false, comment = false;
    for (int i = 0;; ++i) {
        const uint8_t c = s[i];
        if (c == '\n') break;
        if (i == MTX_ML) return mtx::LINE_LONG;                 // MTX_ML bytes and no end
        if (bad || comment) continue;
        if (c == ' ' || c == '\t' || (c == '\r' && s[i + 1] == '\n')) {
            if (indig) {
                if (nf == 0) f0 = v;
                else if (nf == 1) f1 = v;
                else f2 = v;
                over |= (unsigned)(nd > 19) << nf;
                ++nf;
                indig = false;
            }
            continue;
        }
        if (!seen) {
            seen = true;
            if (c == '%') {
                comment = true;
                continue;
            }
        }
        const unsigned d = (unsigned)c - '0';
        if (d <= 9) {
            if (!indig) {
                if (nf == 3) {
                    bad = mtx::LINE_FIELDS;
                    continue;
                }
                indig = true;
                v = 0;
                nd = 0;
            }
            if (nd > 0 || d > 0)
                if (++nd <= 19) v = v * 10 + d;
        } else
            bad = (c == '.' || ((c == 'e' || c == 'E') && indig)) ? mtx::LINE_REAL : mtx::LINE_SYNTAX;
    }
    if (bad) return bad;
    if (comment || !seen) return mtx::LINE_SKIP;
    if (indig) {
        if (nf == 0) f0 = v;
        else if (nf == 1) f1 = v;
        else f2 = v;
        over |= (unsigned)(nd > 19) << nf;
        ++nf;
    }
    if (nf != 3) return mtx::LINE_FIELDS;
    if ((over & 1) || f0 < 1 || f0 > (uint64_t)n_genes) return mtx::LINE_GENE;
    if ((over & 2) || f1 < 1 || f1 > (uint64_t)n_cells) return mtx::LINE_CELL;
    if ((over & 4) || f2 > 0xFFFFFFFFull) return mtx::LINE_VALUE;
    *key = (f1 - 1) << 32 | (f0 - 1);
    *val = (uint32_t)f2;
    return mtx::LINE_ENTRY;
}

__global__ __launch_bounds__(MTX_BLOCK) void mtx_parse_kernel(const uint4 *__restrict__ text, int64_t len, int64_t n_genes, int64_t n_cells,
                                                              uint64_t *__restrict__ stage_key, uint32_t *__restrict__ stage_val,
                                                              uint32_t *__restrict__ tile_count, MtxPieceResult *__restrict__ res)
{
    __shared__ uint4 s_text[MTX_LDS_PIECES];
    __shared__ __attribute__((aligned(8))) uint16_t s_mask[MTX_TILE / 16];
    __shared__ uint64_t s_key[MTX_LANE_ENTRIES * MTX_BLOCK];
    __shared__ uint32_t s_val[MTX_LANE_ENTRIES * MTX_BLOCK];
    __shared__ uint32_t s_wave[MTX_BLOCK / 64];
    const int tid = threadIdx.x;
    const int64_t tile0 = (int64_t)blockIdx.x * MTX_TILE;
    const int64_t n_pieces = (len + 15) / 16, piece0 = tile0 / 16 - 1;
    for (int k = tid; k < MTX_LDS_PIECES; k += MTX_BLOCK) {
        const int64_t gp = piece0 + k;
        uint4 p = make_uint4(0, 0, 0, 0);
        if (gp < 0) p.w = 0x0A000000u;                          // in front of the piece: a `\n`, so that byte 0 starts a line
        else if (gp < n_pieces) p = text[gp];
        s_text[k] = p;
        if (k >= 1 && k <= MTX_TILE / 16)
            s_mask[k - 1] = (uint16_t)(mtx_nl4(p.x) | mtx_nl4(p.y) << 4 | mtx_nl4(p.z) << 8 | mtx_nl4(p.w) << 12);
    }
    __syncthreads();
    const uint8_t *sb = reinterpret_cast<const uint8_t *>(s_text);
    const int lane0 = MTX_LEAD + MTX_LANE_BYTES * tid;          // LDS offset of the lane's first byte
    const uint2 m2 = *reinterpret_cast<const uint2 *>(&s_mask[4 * tid]);
    const uint64_t nl = (uint64_t)m2.y << 32 | m2.x;
    uint64_t starts = nl << 1 | (uint64_t)(sb[lane0 - 1] == '\n');
    const int64_t left = len - (tile0 + (int64_t)MTX_LANE_BYTES * tid);   // a line starts at a byte of the piece only
    if (left <= 0) starts = 0;
    else if (left < 64) starts &= ((uint64_t)1 << left) - 1;
    const uint32_t n_starts = (uint32_t)__popcll(starts);
    uint32_t n_ent = 0;
    unsigned long long err = ~0ull;
    while (starts) {
        const int j = __ffsll((unsigned long long)starts) - 1;
        starts &= starts - 1;
        uint64_t key = 0;
        uint32_t val = 0;
        const int code = mtx_parse_line(sb + lane0 + j, n_genes, n_cells, &key, &val);
        if (code == mtx::LINE_ENTRY && n_ent < MTX_LANE_ENTRIES) {      // (always below: the shortest entry line has 6 bytes)
            s_key[n_ent * MTX_BLOCK + tid] = key;
            s_val[n_ent * MTX_BLOCK + tid] = val;
            ++n_ent;
        } else if (code > 0) {
            const unsigned long long e = (unsigned long long)(tile0 + MTX_LANE_BYTES * tid + j) << 8 | (unsigned)code;
            err = e < err ? e : err;
        }
    }
    if (err != ~0ull) atomicMin(&res->err, err);
    // place of the lane's entries in the tile: lines << 16 | entries, scanned over the workgroup (16384 lines at most)
    uint32_t inc = n_starts << 16 | n_ent;
    const int ln = tid & 63, w = tid >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(inc, d, 64);
        if (ln >= d) inc += y;
    }
    if (ln == 63) s_wave[w] = inc;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int i = 0; i < MTX_BLOCK / 64; ++i) {
        before += i < w ? s_wave[i] : 0;
        total += s_wave[i];
    }
    const uint32_t off = (before + inc - (n_starts << 16 | n_ent)) & 0xFFFFu;
    const int64_t base = (int64_t)blockIdx.x * MTX_TILE_ENTRIES + off;
    for (uint32_t i = 0; i < n_ent; ++i) {
        stage_key[base + i] = s_key[i * MTX_BLOCK + tid];
        stage_val[base + i] = s_val[i * MTX_BLOCK + tid];
    }
    if (tid == 0) {
        tile_count[blockIdx.x] = total & 0xFFFFu;
        atomicAdd(&res->n_lines, (unsigned long long)(total >> 16));
    }
}

__global__ __launch_bounds__(256) void mtx_place_kernel(const uint64_t *__restrict__ stage_key, const uint32_t *__restrict__ stage_val,
                                                        const uint32_t *__restrict__ tile_count, const uint32_t *__restrict__ tile_base,
                                                        int64_t done, int64_t nnz, uint64_t *__restrict__ out_key, uint32_t *__restrict__ out_val)
{
    const int64_t from = (int64_t)blockIdx.x * MTX_TILE_ENTRIES, to = done + tile_base[blockIdx.x];
    const uint32_t n = tile_count[blockIdx.x];
    for (uint32_t i = threadIdx.x; i < n; i += 256)
        if (to + i < nnz) {
            out_key[to + i] = stage_key[from + i];
            out_val[to + i] = stage_val[from + i];
        }
}

hipError_t mtx_scan_temp_bytes(int64_t n_tiles, size_t *bytes)
{
    *bytes = 0;
    return rocprim::exclusive_scan(nullptr, *bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr, 0u, (size_t)(n_tiles + 1),
                                   rocprim::plus<uint32_t>(), (hipStream_t) nullptr);
}

hipError_t mtx_parse_launch(const uint8_t *text, int64_t len, int64_t n_genes, int64_t n_cells, uint64_t *stage_key, uint32_t *stage_val,
                            uint32_t *tile_count, uint32_t *tile_base, void *temp, size_t temp_bytes, int64_t done, int64_t nnz,
                            uint64_t *out_key, uint32_t *out_val, MtxPieceResult *res, hipStream_t st)
{
    const int64_t n_tiles = (len + MTX_TILE - 1) / MTX_TILE;
    hipError_t e = hipMemsetAsync(res, 0xFF, sizeof(unsigned long long), st);
    if (e == hipSuccess) e = hipMemsetAsync(&res->n_lines, 0, sizeof(unsigned long long), st);
    if (e == hipSuccess) e = hipMemsetAsync(tile_count + n_tiles, 0, sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    if (n_tiles > 0)
        hipLaunchKernelGGL(mtx_parse_kernel, dim3((unsigned)n_tiles), dim3(MTX_BLOCK), 0, st, reinterpret_cast<const uint4 *>(text), len, n_genes,
                           n_cells, stage_key, stage_val, tile_count, res);
    e = rocprim::exclusive_scan(temp, temp_bytes, (const uint32_t *)tile_count, tile_base, 0u, (size_t)(n_tiles + 1), rocprim::plus<uint32_t>(), st);
    if (e != hipSuccess) return e;
    if (n_tiles > 0)
        hipLaunchKernelGGL(mtx_place_kernel, dim3((unsigned)n_tiles), dim3(256), 0, st, (const uint64_t *)stage_key, (const uint32_t *)stage_val,
                           (const uint32_t *)tile_count, (const uint32_t *)tile_base, done, nnz, out_key, out_val);
    return hipGetLastError();
}

// the bits of the indices 0 .. n - 1
static unsigned mtx_bits(int64_t n)
{
    unsigned b = 1;
    while (b < 32 && ((int64_t)1 << b) < n) ++b;
    return b;
}

hipError_t mtx_sort_temp_bytes(int64_t nnz, int64_t n_major, int64_t n_minor, size_t *bytes)
{
    rocprim::double_buffer<uint64_t> k(nullptr, nullptr);
    rocprim::double_buffer<uint32_t> v(nullptr, nullptr);
    size_t a = 0, b = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, a, k, v, (size_t)nnz, 0u, mtx_bits(n_minor), (hipStream_t) nullptr);
    if (e == hipSuccess) e = rocprim::radix_sort_pairs(nullptr, b, k, v, (size_t)nnz, 32u, 32u + mtx_bits(n_major), (hipStream_t) nullptr);
    *bytes = a > b ? a : b;
    return e;
}

hipError_t mtx_sort_launch(uint64_t *key[2], uint32_t *val[2], int *which, int64_t nnz, int64_t n_major, int64_t n_minor, bool with_major,
                           void *temp, size_t temp_bytes, hipStream_t st)
{
    if (nnz <= 0) return hipSuccess;
    rocprim::double_buffer<uint64_t> k(key[*which], key[1 - *which]);
    rocprim::double_buffer<uint32_t> v(val[*which], val[1 - *which]);
    hipError_t e = rocprim::radix_sort_pairs(temp, temp_bytes, k, v, (size_t)nnz, 0u, mtx_bits(n_minor), st);
    if (e == hipSuccess && with_major) e = rocprim::radix_sort_pairs(temp, temp_bytes, k, v, (size_t)nnz, 32u, 32u + mtx_bits(n_major), st);
    *which = k.current() == key[0] ? 0 : 1;
    return e;
}

__global__ __launch_bounds__(256) void mtx_dup_kernel(const uint64_t *__restrict__ keys, int64_t nnz, unsigned long long *__restrict__ dup)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x + 1;
    if (i < nnz && keys[i] == keys[i - 1]) atomicMin(dup, (unsigned long long)keys[i]);
}

hipError_t mtx_dup_launch(const uint64_t *keys, int64_t nnz, unsigned long long *dup, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(dup, 0xFF, sizeof(unsigned long long), st);
    if (e != hipSuccess || nnz < 2) return e;
    hipLaunchKernelGGL(mtx_dup_kernel, dim3((unsigned)((nnz + 254) / 256)), dim3(256), 0, st, keys, nnz, dup);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void mtx_split_kernel(const uint64_t *__restrict__ keys, int64_t nnz, uint32_t *__restrict__ lo, uint32_t *__restrict__ hi)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nnz) return;
    const uint64_t k = keys[i];
    if (lo) lo[i] = (uint32_t)k;
    if (hi) hi[i] = (uint32_t)(k >> 32);
}

hipError_t mtx_split_launch(const uint64_t *keys, int64_t nnz, uint32_t *lo, uint32_t *hi, hipStream_t st)
{
    if (nnz <= 0) return hipSuccess;
    hipLaunchKernelGGL(mtx_split_kernel, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, st, keys, nnz, lo, hi);
    return hipGetLastError();
}

// the row of entry e: the last r with ptr[r] <= e (empty rows have ptr[r] = ptr[r + 1] and are stepped over)
__global__ __launch_bounds__(256) void mtx_expand_kernel(const int64_t *__restrict__ ptr, int64_t n_rows, const int32_t *__restrict__ idx, int64_t nnz,
                                                         uint64_t *__restrict__ keys)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nnz) return;
    int64_t lo = 0, hi = n_rows;                                // ptr[lo] <= e < ptr[hi]
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (ptr[mid] <= e) lo = mid;
        else hi = mid;
    }
    keys[e] = (uint64_t)lo << 32 | (uint32_t)idx[e];
}

hipError_t mtx_expand_launch(const int64_t *ptr, int64_t n_rows, const int32_t *idx, int64_t nnz, uint64_t *keys, hipStream_t st)
{
    if (nnz <= 0) return hipSuccess;
    hipLaunchKernelGGL(mtx_expand_kernel, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, st, ptr, n_rows, idx, nnz, keys);
    return hipGetLastError();
}

}  // namespace nabo

// ---- the C ABI --------------------------------------------------------------------------------------------------------
using nabo::DevBuf;
namespace mtx = nabo::mtx;

struct nabo_mtx {
    int device = 0;
    int64_t budget = 0;
    mtx::HeaderParser head;
    mtx::LineBuffer lines;
    uint8_t *pinned = nullptr;
    bool allocated = false, finished = false, failed = false;
    int64_t lines_done = 0, entries_done = 0, n_chunks = 0;
    int64_t n_tiles_cap = 0;
    double ms[5] = {0, 0, 0, 0, 0};
    nabo::Events<4> ev;
    DevBuf d_text, d_stage_key, d_stage_val, d_count, d_base, d_temp, d_res, d_key[2], d_val[2], d_gene, d_csr_val, d_cell_ptr, d_gene_ptr;
    int which = 0;
    ~nabo_mtx()
    {
        if (pinned) (void)hipHostFree(pinned);
    }
};

namespace {

int64_t mtx_peak_bytes(int64_t nnz, int64_t n_genes, int64_t n_cells, const mtx::LineBuffer &lb)
{
    const int64_t C = lb.chunk, t = (C + mtx::MAX_LINE + 1 + mtx::TILE_BYTES - 1) / mtx::TILE_BYTES;
    return 32 * nnz + 8 * (n_cells + 1) + 8 * (n_genes + 1) + (C + mtx::MAX_LINE + 64) + 12 * (int64_t)(mtx::TILE_BYTES / 6 + 2) * t + 8 * (t + 2) + 64;
}

int mtx_fail(nabo_mtx *h, int rc)
{
    h->failed = true;
    return rc;
}

// the size line is known: the budget, then every device buffer of the handle
int mtx_allocate(nabo_mtx *h)
{
    const int64_t nnz = h->head.nnz, n_genes = h->head.n_genes, n_cells = h->head.n_cells;
    const int64_t peak = mtx_peak_bytes(nnz, n_genes, n_cells, h->lines);
    if (peak > h->budget)
        return nabo::api_fail(NABO_E_NOMEM, "nnz = %lld with chunks of %lld bytes needs %lld bytes of device memory, the budget is %lld", (long long)nnz,
                              (long long)h->lines.chunk, (long long)peak, (long long)h->budget);
    int rc = nabo::use_device(h->device);
    if (rc) return rc;
    const int64_t max_piece = h->lines.max_piece();
    h->n_tiles_cap = (max_piece + mtx::TILE_BYTES - 1) / mtx::TILE_BYTES;
    size_t scan = 0, sort = 0;
    HIP_TRY(nabo::mtx_scan_temp_bytes(h->n_tiles_cap, &scan));
    HIP_TRY(nabo::mtx_sort_temp_bytes(nnz, n_cells, n_genes, &sort));
    const size_t temp = std::max(scan, sort);
    if (peak + (int64_t)temp > h->budget)
        return nabo::api_fail(NABO_E_NOMEM, "nnz = %lld with chunks of %lld bytes needs %lld bytes of device memory, the budget is %lld", (long long)nnz,
                              (long long)h->lines.chunk, (long long)(peak + (int64_t)temp), (long long)h->budget);
    HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&h->pinned), (size_t)max_piece, hipHostMallocDefault));
    h->lines.buf = h->pinned;
    HIP_TRY(h->d_text.alloc((size_t)((max_piece + 15) / 16 * 16)));
    HIP_TRY(h->d_stage_key.alloc((size_t)h->n_tiles_cap * nabo::mtx_tile_entries() * 8));
    HIP_TRY(h->d_stage_val.alloc((size_t)h->n_tiles_cap * nabo::mtx_tile_entries() * 4));
    HIP_TRY(h->d_count.alloc((size_t)(h->n_tiles_cap + 1) * 4));
    HIP_TRY(h->d_base.alloc((size_t)(h->n_tiles_cap + 1) * 4));
    HIP_TRY(h->d_temp.alloc(temp));
    HIP_TRY(h->d_res.alloc(sizeof(nabo::MtxPieceResult) + 8));
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(h->d_key[i].alloc((size_t)nnz * 8));
        HIP_TRY(h->d_val[i].alloc((size_t)nnz * 4));
    }
    HIP_TRY(h->d_gene.alloc((size_t)nnz * 4));
    HIP_TRY(h->d_csr_val.alloc((size_t)nnz * 4));
    HIP_TRY(h->d_cell_ptr.alloc((size_t)(n_cells + 1) * 8));
    HIP_TRY(h->d_gene_ptr.alloc((size_t)(n_genes + 1) * 8));
    HIP_TRY(h->ev.create());
    h->allocated = true;
    return NABO_OK;
}

int64_t count_newlines(const uint8_t *p, int64_t n) { return (int64_t)std::count(p, p + n, (uint8_t)'\n'); }

int mtx_line_error(nabo_mtx *h, int64_t line_in_body, int code)
{
    return nabo::api_fail(NABO_E_INVALID, "line %lld: %s", (long long)(h->head.lines + line_in_body), mtx::code_text(code));
}

// upload and parse lines.buf[0, len): whole lines, the last with its `\n`
int mtx_parse_piece(nabo_mtx *h, int64_t len)
{
    if (len <= 0) return NABO_OK;
    hipStream_t st = nullptr;
    const int64_t padded = (len + 15) / 16 * 16, n_tiles = (len + mtx::TILE_BYTES - 1) / mtx::TILE_BYTES;
    nabo::MtxPieceResult res;
    uint32_t n_ent = 0;
    nabo::MtxPieceResult *d_res = h->d_res.as<nabo::MtxPieceResult>();
    HIP_TRY(hipEventRecord(h->ev.ev[0], st));
    HIP_TRY(hipMemcpyAsync(h->d_text.p, h->lines.buf, (size_t)len, hipMemcpyHostToDevice, st));
    if (padded > len) HIP_TRY(hipMemsetAsync(h->d_text.as<uint8_t>() + len, 0, (size_t)(padded - len), st));
    HIP_TRY(hipEventRecord(h->ev.ev[1], st));
    HIP_TRY(nabo::mtx_parse_launch(h->d_text.as<uint8_t>(), len, h->head.n_genes, h->head.n_cells, h->d_stage_key.as<uint64_t>(),
                                   h->d_stage_val.as<uint32_t>(), h->d_count.as<uint32_t>(), h->d_base.as<uint32_t>(), h->d_temp.p, h->d_temp.cap,
                                   h->entries_done, h->head.nnz, h->d_key[0].as<uint64_t>(), h->d_val[0].as<uint32_t>(), d_res, st));
    HIP_TRY(hipEventRecord(h->ev.ev[2], st));
    HIP_TRY(hipMemcpyAsync(&res, d_res, sizeof res, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&n_ent, h->d_base.as<uint32_t>() + n_tiles, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(h->ev.elapsed(0, 1, &h->ms[0]));
    HIP_TRY(h->ev.elapsed(1, 2, &h->ms[1]));
    ++h->n_chunks;
    const uint8_t *buf = h->lines.buf;
    const int64_t bad_at = res.err == ~0ull ? len : (int64_t)(res.err >> 8);
    if (h->entries_done + (int64_t)n_ent > h->head.nnz) {
        // the first entry line in excess, unless a bad line stands in front of it
        int64_t k = h->entries_done, line = h->lines_done, pos = 0;
        while (pos < bad_at) {
            const uint8_t *nl = static_cast<const uint8_t *>(memchr(buf + pos, '\n', (size_t)(len - pos)));
            const int64_t end = nl ? nl - buf : len;
            uint64_t f[3];
            ++line;
            if (mtx::parse_line(buf + pos, end - pos, h->head.n_genes, h->head.n_cells, f) == mtx::LINE_ENTRY && ++k > h->head.nnz)
                return mtx_line_error(h, line, mtx::LINE_EXCESS);
            pos = end + 1;
        }
    }
    if (res.err != ~0ull) return mtx_line_error(h, h->lines_done + count_newlines(buf, bad_at) + 1, (int)(res.err & 0xFF));
    h->lines_done += (int64_t)res.n_lines;
    h->entries_done += n_ent;
    return NABO_OK;
}

int mtx_feed_body(nabo_mtx *h, const uint8_t *p, int64_t n)
{
    while (n > 0) {
        const int64_t took = h->lines.push(p, n);
        p += took, n -= took;
        if (!h->lines.ready()) continue;
        const int64_t len = h->lines.piece();
        if (len == 0) {
            if (h->lines.too_long()) return mtx_line_error(h, h->lines_done + 1, mtx::LINE_LONG);
            continue;
        }
        const int rc = mtx_parse_piece(h, len);
        if (rc) return rc;
        h->lines.drop(len);
    }
    return NABO_OK;
}

int mtx_check_handle(nabo_mtx *h, bool want_finished)
{
    if (!h) return nabo::api_fail(NABO_E_INVALID, "the reader is NULL");
    if (h->failed) return nabo::api_fail(NABO_E_INVALID, "the reader has failed before; only nabo_mtx_free is left");
    if (want_finished != h->finished)
        return nabo::api_fail(NABO_E_INVALID, want_finished ? "nabo_mtx_finish has not been called" : "nabo_mtx_finish has been called already");
    return NABO_OK;
}

int mtx_download(nabo_mtx *h, void *dst, const void *src, size_t bytes)
{
    if (!dst || !bytes) return NABO_OK;
    HIP_TRY(hipEventRecord(h->ev.ev[0], nullptr));
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipEventRecord(h->ev.ev[1], nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(h->ev.elapsed(0, 1, &h->ms[4]));
    return NABO_OK;
}

using nabo::mtx_transpose_stage;                                // (mtx_stages.h: shared with counts.hip)

}  // namespace

extern "C" {

int nabo_mtx_create(int32_t device, int64_t chunk_bytes, int64_t mem_budget_bytes, nabo_mtx **out)
{
    if (!out) return nabo::api_fail(NABO_E_INVALID, "out is NULL");
    *out = nullptr;
    int rc = nabo::use_device(device);
    if (rc) return rc;
    return nabo::create_handle(out, device, "nabo_mtx_create", [&](nabo_mtx *h) {
        h->lines.chunk = mtx::LineBuffer::clamp_chunk(chunk_bytes);
        h->budget = mem_budget_bytes;
        if (mem_budget_bytes <= 0) {
            size_t free_b = 0, total_b = 0;
            HIP_TRY(hipMemGetInfo(&free_b, &total_b));
            h->budget = (int64_t)(free_b / 4 * 3);
        }
        return NABO_OK;
    });
}

int nabo_mtx_feed(nabo_mtx *h, const void *bytes, int64_t n)
{
    int rc = mtx_check_handle(h, false);
    if (rc) return rc;
    if (n < 0 || (n > 0 && !bytes)) return nabo::api_fail(NABO_E_INVALID, "bytes is NULL or n negative");
    const uint8_t *p = static_cast<const uint8_t *>(bytes);
    try {
        if (!h->head.done) {
            const int64_t took = h->head.feed(p, n);
            if (h->head.status) return mtx_fail(h, nabo::api_fail(h->head.status, "%s", h->head.message.c_str()));
            p += took, n -= took;
            if (!h->head.done) return NABO_OK;
            if ((rc = mtx_allocate(h))) return mtx_fail(h, rc);
        }
        if ((rc = nabo::use_device(h->device))) return mtx_fail(h, rc);
        if ((rc = mtx_feed_body(h, p, n))) return mtx_fail(h, rc);
    } catch (const std::bad_alloc &) {
        return mtx_fail(h, nabo::api_fail(NABO_E_NOMEM, "nabo_mtx_feed: out of host memory"));
    }
    return NABO_OK;
}

int nabo_mtx_finish(nabo_mtx *h, int64_t *n_genes, int64_t *n_cells, int64_t *nnz_out)
{
    int rc = mtx_check_handle(h, false);
    if (rc) return rc;
    try {
        if (!h->head.done) {
            if (h->head.finish()) return mtx_fail(h, nabo::api_fail(h->head.status, "%s", h->head.message.c_str()));
            if ((rc = mtx_allocate(h))) return mtx_fail(h, rc);
        }
    } catch (const std::bad_alloc &) {
        return mtx_fail(h, nabo::api_fail(NABO_E_NOMEM, "nabo_mtx_finish: out of host memory"));
    }
    if ((rc = nabo::use_device(h->device))) return mtx_fail(h, rc);
    if ((rc = mtx_parse_piece(h, h->lines.close()))) return mtx_fail(h, rc);
    h->lines.size = 0;
    const int64_t nnz = h->head.nnz, n_g = h->head.n_genes, n_c = h->head.n_cells;
    if (h->entries_done != nnz)
        return mtx_fail(h, nabo::api_fail(NABO_E_INVALID, "line %lld: the file ends after %lld entry lines, the size line announced %lld",
                                          (long long)(h->head.lines + h->lines_done), (long long)h->entries_done, (long long)nnz));
    hipStream_t st = nullptr;
    uint64_t *k[2] = {h->d_key[0].as<uint64_t>(), h->d_key[1].as<uint64_t>()};
    uint32_t *v[2] = {h->d_val[0].as<uint32_t>(), h->d_val[1].as<uint32_t>()};
    unsigned long long dup = ~0ull, *d_dup = reinterpret_cast<unsigned long long *>(h->d_res.as<uint8_t>() + sizeof(nabo::MtxPieceResult));
    auto run = [&]() -> int {
        HIP_TRY(hipEventRecord(h->ev.ev[0], st));
        HIP_TRY(nabo::mtx_sort_launch(k, v, &h->which, nnz, n_c, n_g, true, h->d_temp.p, h->d_temp.cap, st));
        HIP_TRY(nabo::mtx_dup_launch(k[h->which], nnz, d_dup, st));
        if (nnz > 0) HIP_TRY(nabo::key_rowptr_launch(k[h->which], nnz, n_c, h->d_cell_ptr.as<int64_t>(), st));
        else HIP_TRY(hipMemsetAsync(h->d_cell_ptr.p, 0, (size_t)(n_c + 1) * 8, st));
        HIP_TRY(nabo::mtx_split_launch(k[h->which], nnz, h->d_gene.as<uint32_t>(), nullptr, st));
        if (nnz > 0) HIP_TRY(hipMemcpyAsync(h->d_csr_val.p, v[h->which], (size_t)nnz * 4, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipEventRecord(h->ev.ev[1], st));
        HIP_TRY(hipMemcpyAsync(&dup, d_dup, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(h->ev.elapsed(0, 1, &h->ms[2]));
        return NABO_OK;
    };
    if ((rc = run())) return mtx_fail(h, rc);
    if (dup != ~0ull)
        return mtx_fail(h, nabo::api_fail(NABO_E_INVALID, "gene %llu of cell %llu is listed more than once", (dup & 0xFFFFFFFFull) + 1, (dup >> 32) + 1));
    auto transpose = [&]() -> int {
        uint32_t *cells = nullptr;
        HIP_TRY(hipEventRecord(h->ev.ev[0], st));
        const int r = mtx_transpose_stage(h->d_key, h->d_val, &h->which, nnz, n_c, n_g, h->d_temp.p, h->d_temp.cap, h->d_gene_ptr.as<int64_t>(), &cells, st);
        if (r) return r;
        HIP_TRY(hipEventRecord(h->ev.ev[1], st));
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(h->ev.elapsed(0, 1, &h->ms[3]));
        return NABO_OK;
    };
    if ((rc = transpose())) return mtx_fail(h, rc);
    h->finished = true;
    if (n_genes) *n_genes = n_g;
    if (n_cells) *n_cells = n_c;
    if (nnz_out) *nnz_out = nnz;
    return NABO_OK;
}

int nabo_mtx_get_csr(nabo_mtx *h, int64_t *cell_ptr, int32_t *gene, uint32_t *val)
{
    int rc = mtx_check_handle(h, true);
    if (rc || (rc = nabo::use_device(h->device))) return rc;
    const size_t nnz = (size_t)h->head.nnz;
    if ((rc = mtx_download(h, cell_ptr, h->d_cell_ptr.p, (size_t)(h->head.n_cells + 1) * 8))) return rc;
    if ((rc = mtx_download(h, gene, h->d_gene.p, nnz * 4))) return rc;
    return mtx_download(h, val, h->d_csr_val.p, nnz * 4);
}

int nabo_mtx_get_csc(nabo_mtx *h, int64_t *gene_ptr, int32_t *cell, uint32_t *val)
{
    int rc = mtx_check_handle(h, true);
    if (rc || (rc = nabo::use_device(h->device))) return rc;
    const size_t nnz = (size_t)h->head.nnz;
    if ((rc = mtx_download(h, gene_ptr, h->d_gene_ptr.p, (size_t)(h->head.n_genes + 1) * 8))) return rc;
    if ((rc = mtx_download(h, cell, h->d_key[1 - h->which].p, nnz * 4))) return rc;
    return mtx_download(h, val, h->d_val[h->which].p, nnz * 4);
}

void nabo_mtx_free(nabo_mtx *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    delete h;
}

int nabo_mtx_geometry(int32_t *tile_bytes, int32_t *max_line)
{
    if (!tile_bytes || !max_line) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    *tile_bytes = mtx::TILE_BYTES;
    *max_line = mtx::MAX_LINE;
    return NABO_OK;
}

int nabo_mtx_last_device_ms(nabo_mtx *h, double ms[5], int64_t *n_chunks)
{
    if (!h || !ms) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    for (int i = 0; i < 5; ++i) ms[i] = h->ms[i];
    if (n_chunks) *n_chunks = h->n_chunks;
    return NABO_OK;
}

int nabo_csr_transpose(int32_t device, int64_t n_rows, int64_t n_cols, const int64_t *ptr, const int32_t *idx, const float *val, int64_t *out_ptr,
                       int32_t *out_idx, float *out_val)
{
    if (n_rows < 0 || n_rows >= ((int64_t)1 << 31) - 1) return nabo::api_fail(NABO_E_INVALID, "n_rows=%lld out of range [0, 2^31 - 1)", (long long)n_rows);
    if (n_cols < 0 || n_cols >= ((int64_t)1 << 31) - 1) return nabo::api_fail(NABO_E_INVALID, "n_cols=%lld out of range [0, 2^31 - 1)", (long long)n_cols);
    int rc = nabo::check_sparse<nabo::SPARSE_RAW>(nullptr, "row", "column", n_rows, n_cols, ptr, idx, val, nullptr, true);
    if (rc) return rc;
    const int64_t nnz = ptr[n_rows];
    if (nnz >= 0xFFFFFFFFll) return nabo::api_fail(NABO_E_UNSUPPORTED, "nnz=%lld must be below 2^32 - 1", (long long)nnz);
    if (!out_ptr || (nnz > 0 && (!out_idx || !out_val))) return nabo::api_fail(NABO_E_INVALID, "an output array is NULL");
    if ((rc = nabo::use_device(device))) return rc;
    hipStream_t st = nullptr;
    DevBuf key[2], v[2], d_ptr, d_out_ptr, d_temp;
    size_t temp = 0;
    HIP_TRY(nabo::mtx_sort_temp_bytes(nnz, n_rows, n_cols, &temp));
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(key[i].alloc((size_t)nnz * 8));
        HIP_TRY(v[i].alloc((size_t)nnz * 4));
    }
    HIP_TRY(d_ptr.alloc((size_t)(n_rows + 1) * 8));
    HIP_TRY(d_out_ptr.alloc((size_t)(n_cols + 1) * 8));
    HIP_TRY(d_temp.alloc(temp));
    HIP_TRY(hipMemcpyAsync(d_ptr.p, ptr, (size_t)(n_rows + 1) * 8, hipMemcpyHostToDevice, st));
    if (nnz > 0) {
        HIP_TRY(hipMemcpyAsync(key[1].p, idx, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(v[0].p, val, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(nabo::mtx_expand_launch(d_ptr.as<int64_t>(), n_rows, key[1].as<int32_t>(), nnz, key[0].as<uint64_t>(), st));
    int which = 0;
    uint32_t *rows = nullptr;
    if ((rc = mtx_transpose_stage(key, v, &which, nnz, n_rows, n_cols, d_temp.p, d_temp.cap, d_out_ptr.as<int64_t>(), &rows, st))) return rc;
    HIP_TRY(hipMemcpyAsync(out_ptr, d_out_ptr.p, (size_t)(n_cols + 1) * 8, hipMemcpyDeviceToHost, st));
    if (nnz > 0) {
        HIP_TRY(hipMemcpyAsync(out_idx, rows, (size_t)nnz * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_val, v[which].p, (size_t)nnz * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return NABO_OK;
}

}  // extern "C"
