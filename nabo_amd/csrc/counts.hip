// Count matrices out and across (include/nabo_counts.h is the specification): the Matrix Market writer, the mirror of
// mtx_ingest.hip, and the remap behind subsetting and merging.
//
// WRITER.  The length pass gives every entry the offset of its line inside its cell and every cell its bytes: a group of
// 16 lanes walks one cell 16 entries at a time with a running prefix (mtxw_len_kernel), a cell of more than LONG_CELL
// entries is walked by a workgroup (mtxw_len_long_kernel).  A rocPRIM exclusive scan makes 64-bit cell offsets of the bytes.
// mtxw_format_kernel: one workgroup owns CW_TILE bytes of the body.  It finds the cells that have a byte in its tile by
// binary search over the cell offsets and the first and last line by binary search over the entry offsets of the two end
// cells; the lines in between are consecutive entries of the CSR, one per lane and step, whose cell is found among the
// tile's cells.  A lane writes its line into LDS backwards from its end, and the workgroup stores its tile -- nothing
// else -- with 16-byte stores.  The line that holds the tile's first byte began in the tile before: it is formatted here as
// well, into CW_LEAD bytes in front of the tile in LDS that are never stored, and the line that runs over the tile's end
// spills into as many bytes behind it.  So a straddling line is formatted twice and every byte of the text is stored once.
//
// REMAP.  16 lanes per output row count what col_map keeps, a scan places the rows, the same lanes write (row << 32 |
// new column, value); the sort, the duplicate check and the transpose are the reader's stages (launch.h, mtx_stages.h).
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/nabo_counts.h"
#include "counts_host.h"
#include "host_common.h"
#include "launch.h"
#include "mtx_stages.h"

namespace nabo {

namespace cnt = counts;

constexpr int CW_TILE = cnt::TILE_BYTES, CW_BLOCK = 256, CW_GROUP = 16, CW_LEAD = 48;
constexpr int CW_LDS = CW_LEAD + CW_TILE + 48;                   // a line has at most 33 bytes on either side of the tile
static_assert(CW_LEAD % 16 == 0 && CW_TILE % 16 == 0 && CW_LEAD >= cnt::MAX_LINE, "whole 16-byte pieces; room for a line in front");

// inclusive prefix sum over the W lanes of a group
template <int W> __device__ __forceinline__ uint32_t group_scan(uint32_t x, int lane)
{
#pragma unroll
    for (int d = 1; d < W; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, W);
        if (lane >= d) x += y;
    }
    return x;
}

// ent_off[e]: the offset of entry e's line from the start of its cell; cell_len[c]: the bytes of cell c.  Cells of more
// than LONG_CELL entries are left to mtxw_len_long_kernel.
__global__ __launch_bounds__(CW_BLOCK) void mtxw_len_kernel(const int64_t *__restrict__ ptr, const int32_t *__restrict__ gene,
                                                            const uint32_t *__restrict__ val, int64_t n_cells, int blank,
                                                            uint32_t *__restrict__ ent_off, uint64_t *__restrict__ cell_len)
{
    const int lane = threadIdx.x & (CW_GROUP - 1);
    const int64_t c = (int64_t)blockIdx.x * (CW_BLOCK / CW_GROUP) + threadIdx.x / CW_GROUP;
    const bool live = c < n_cells;
    const int64_t e0 = live ? ptr[c] : 0, n = live ? ptr[c + 1] - e0 : 0;
    const int64_t e1 = n > cnt::LONG_CELL ? e0 : e0 + n;
    uint32_t running = 0;
    for (int64_t b = e0; b < e1; b += CW_GROUP) {
        const int64_t e = b + lane;
        const uint32_t len = e < e1 ? (uint32_t)cnt::line_bytes((uint32_t)gene[e], (uint32_t)c, val[e]) : 0u;
        const uint32_t incl = group_scan<CW_GROUP>(len, lane);
        if (e < e1) ent_off[e] = running + incl - len;
        running += __shfl(incl, CW_GROUP - 1, CW_GROUP);
    }
    if (live && lane == 0 && n <= cnt::LONG_CELL) cell_len[c] = n == 0 ? (blank ? 1u : 0u) : running;
}

__global__ __launch_bounds__(CW_BLOCK) void mtxw_len_long_kernel(const int64_t *__restrict__ ptr, const int32_t *__restrict__ gene,
                                                                 const uint32_t *__restrict__ val, const int32_t *__restrict__ cells,
                                                                 uint32_t *__restrict__ ent_off, uint64_t *__restrict__ cell_len)
{
    __shared__ uint32_t s_wave[CW_BLOCK / 64];
    const int tid = threadIdx.x, ln = tid & 63, w = tid >> 6;
    const int64_t c = cells[blockIdx.x], e0 = ptr[c], e1 = ptr[c + 1];
    uint32_t running = 0;
    for (int64_t b = e0; b < e1; b += CW_BLOCK) {
        const int64_t e = b + tid;
        const uint32_t len = e < e1 ? (uint32_t)cnt::line_bytes((uint32_t)gene[e], (uint32_t)c, val[e]) : 0u;
        const uint32_t incl = group_scan<64>(len, ln);
        if (ln == 63) s_wave[w] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int i = 0; i < CW_BLOCK / 64; ++i) {
            before += i < w ? s_wave[i] : 0u;
            total += s_wave[i];
        }
        if (e < e1) ent_off[e] = running + before + incl - len;
        running += total;
        __syncthreads();
    }
    if (tid == 0) cell_len[c] = running;
}

// The body bytes [body0, body0 + len) to out (16-byte pieces, out[0] is byte body0; body0 is a whole number of tiles into
// the chunk's buffer by construction: one workgroup per tile of the chunk).  cell_off [n_cells + 1].
__global__ __launch_bounds__(CW_BLOCK) void mtxw_format_kernel(const int64_t *__restrict__ ptr, const int32_t *__restrict__ gene,
                                                               const uint32_t *__restrict__ val, const uint32_t *__restrict__ ent_off,
                                                               const uint64_t *__restrict__ cell_off, int64_t n_cells, int blank, int64_t body0,
                                                               int64_t len, uint4 *__restrict__ out)
{
    __shared__ uint4 s_text[CW_LDS / 16];
    uint8_t *sb = reinterpret_cast<uint8_t *>(s_text);
    const int tid = threadIdx.x;
    const int64_t a0 = body0 + (int64_t)blockIdx.x * CW_TILE;
    const int64_t a1 = a0 + CW_TILE < body0 + len ? a0 + CW_TILE : body0 + len;
    // c0: the last cell that starts at or in front of a0 (cells without bytes are stepped over); c1: the last that starts in front of a1
    int64_t lo = 0, hi = n_cells;                               // cell_off[lo] <= a0 < cell_off[hi]
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if ((int64_t)cell_off[mid] <= a0) lo = mid;
        else hi = mid;
    }
    const int64_t c0 = lo;
    hi = n_cells;                                               // cell_off[lo] < a1 <= cell_off[hi]
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if ((int64_t)cell_off[mid] < a1) lo = mid;
        else hi = mid;
    }
    const int64_t c1 = lo;
    // e0: the entry of c0 whose line holds byte a0; e1: the first entry of c1 whose line starts at or behind a1
    int64_t e0 = ptr[c0];
    {
        const int64_t p1 = ptr[c0 + 1], rel = a0 - (int64_t)cell_off[c0];
        int64_t h = p1;                                         // ent_off[e0] <= rel < ent_off[h]
        while (h - e0 > 1) {
            const int64_t mid = e0 + (h - e0) / 2;
            if ((int64_t)ent_off[mid] <= rel) e0 = mid;
            else h = mid;
        }
    }
    int64_t e1 = ptr[c1];
    {
        const int64_t rel = a1 - (int64_t)cell_off[c1];
        int64_t h = ptr[c1 + 1];
        while (e1 < h) {
            const int64_t mid = e1 + (h - e1) / 2;
            if ((int64_t)ent_off[mid] < rel) e1 = mid + 1;
            else h = mid;
        }
    }
    // the `\n` of every cell without entries (then every cell has a byte, and the tile holds CW_TILE + 1 cells at most)
    if (blank)
        for (int64_t c = c0 + tid; c <= c1; c += CW_BLOCK) {
            const int64_t at = (int64_t)cell_off[c] - a0;
            if (ptr[c] == ptr[c + 1] && at >= 0 && at < a1 - a0) sb[CW_LEAD + at] = (uint8_t)'\n';
        }
    for (int64_t e = e0 + tid; e < e1; e += CW_BLOCK) {
        int64_t cl = c0, ch = c1 + 1;                           // ptr[cl] <= e < ptr[ch]
        while (ch - cl > 1) {
            const int64_t mid = cl + (ch - cl) / 2;
            if (ptr[mid] <= e) cl = mid;
            else ch = mid;
        }
        const uint32_t g = (uint32_t)gene[e], v = val[e];
        const int64_t start = CW_LEAD + ((int64_t)cell_off[cl] + (int64_t)ent_off[e] - a0);
        const int64_t end = start + cnt::line_bytes(g, (uint32_t)cl, v);
        if (start >= 0 && end <= CW_LDS) cnt::put_line(sb + end, g, (uint32_t)cl, v);      // (always: the line has a byte in the tile)
    }
    __syncthreads();
    const int n_pieces = (int)((a1 - a0 + 15) / 16);
    uint4 *dst = out + (int64_t)blockIdx.x * (CW_TILE / 16);
    for (int k = tid; k < n_pieces; k += CW_BLOCK) dst[k] = s_text[CW_LEAD / 16 + k];
}

// what col_map keeps of output row r = input row row_src[r]: counted, and written as keys from out_ptr[r] on
__global__ __launch_bounds__(CW_BLOCK) void remap_count_kernel(const int64_t *__restrict__ ptr, const int32_t *__restrict__ idx,
                                                               const int64_t *__restrict__ row_src, const int32_t *__restrict__ col_map,
                                                               int64_t n_out_rows, int64_t *__restrict__ count)
{
    const int lane = threadIdx.x & (CW_GROUP - 1);
    const int64_t r = (int64_t)blockIdx.x * (CW_BLOCK / CW_GROUP) + threadIdx.x / CW_GROUP;
    const bool live = r < n_out_rows;
    const int64_t s = live ? row_src[r] : 0, e0 = live ? ptr[s] : 0, e1 = live ? ptr[s + 1] : 0;
    uint32_t n = 0;
    for (int64_t e = e0 + lane; e < e1; e += CW_GROUP) n += col_map[idx[e]] >= 0;
#pragma unroll
    for (int d = CW_GROUP / 2; d > 0; d >>= 1) n += __shfl_xor(n, d, CW_GROUP);
    if (live && lane == 0) count[r] = n;
}

__global__ __launch_bounds__(CW_BLOCK) void remap_write_kernel(const int64_t *__restrict__ ptr, const int32_t *__restrict__ idx,
                                                               const uint32_t *__restrict__ val, const int64_t *__restrict__ row_src,
                                                               const int32_t *__restrict__ col_map, int64_t n_out_rows,
                                                               const int64_t *__restrict__ out_ptr, uint64_t *__restrict__ key,
                                                               uint32_t *__restrict__ out_val)
{
    const int lane = threadIdx.x & (CW_GROUP - 1);
    const int64_t r = (int64_t)blockIdx.x * (CW_BLOCK / CW_GROUP) + threadIdx.x / CW_GROUP;
    const bool live = r < n_out_rows;
    const int64_t s = live ? row_src[r] : 0, e0 = live ? ptr[s] : 0, e1 = live ? ptr[s + 1] : 0;
    int64_t at = live ? out_ptr[r] : 0;
    for (int64_t b = e0; b < e1; b += CW_GROUP) {
        const int64_t e = b + lane;
        const int32_t m = e < e1 ? col_map[idx[e]] : -1;
        const uint32_t keep = m >= 0, incl = group_scan<CW_GROUP>(keep, lane);
        if (keep) {
            key[at + incl - 1] = (uint64_t)r << 32 | (uint32_t)m;
            out_val[at + incl - 1] = val[e];
        }
        at += __shfl(incl, CW_GROUP - 1, CW_GROUP);
    }
}

static hipError_t scan_u64_temp_bytes(int64_t n, size_t *bytes)
{
    *bytes = 0;
    return rocprim::exclusive_scan(nullptr, *bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t)0, (size_t)n, rocprim::plus<uint64_t>(),
                                   (hipStream_t) nullptr);
}

static hipError_t scan_u64_launch(void *temp, size_t temp_bytes, const uint64_t *in, uint64_t *out, int64_t n, hipStream_t st)
{
    return rocprim::exclusive_scan(temp, temp_bytes, in, out, (uint64_t)0, (size_t)n, rocprim::plus<uint64_t>(), st);
}

static unsigned groups_grid(int64_t n) { return (unsigned)((n + CW_BLOCK / CW_GROUP - 1) / (CW_BLOCK / CW_GROUP)); }

}  // namespace nabo

// ---- the C ABI --------------------------------------------------------------------------------------------------------
using nabo::DevBuf;
namespace cnt = nabo::counts;

struct nabo_mtxw {
    int device = 0;
    int64_t n_cells = 0, nnz = 0, chunk = 0, n_chunks = 0;
    int blank = 0;
    bool failed = false;
    cnt::Server srv;
    uint8_t *pinned = nullptr;
    double ms[4] = {0, 0, 0, 0};
    nabo::Events<3> ev;
    DevBuf d_ptr, d_gene, d_val, d_ent_off, d_len, d_off, d_long, d_temp, d_text;
    ~nabo_mtxw()
    {
        if (pinned) (void)hipHostFree(pinned);
    }
};

namespace {

int index_fail(const cnt::IdxVerdict &v, const char *major, const char *minor, int64_t n_minor, const int32_t *idx)
{
    if (v.code == cnt::IDX_NULL) return nabo::api_fail(NABO_E_INVALID, "%s or val is NULL", minor);
    if (v.code == cnt::IDX_RANGE)
        return nabo::api_fail(NABO_E_INVALID, "%s[%lld] = %lld is not a %s in [0, %lld)", minor, (long long)v.entry, (long long)idx[v.entry], minor,
                              (long long)n_minor);
    return nabo::api_fail(NABO_E_INVALID, "the %ss of %s %lld are not strictly increasing at entry %lld", minor, major, (long long)v.major, (long long)v.entry);
}

int size_check(const char *name, int64_t v, int64_t limit, const char *limit_text)
{
    if (v < 0) return nabo::api_fail(NABO_E_INVALID, "%s=%lld is negative", name, (long long)v);
    if (v >= limit) return nabo::api_fail(NABO_E_UNSUPPORTED, "%s=%lld must be below %s", name, (long long)v, limit_text);
    return NABO_OK;
}

// uploads the matrix, runs the length pass and the scan; h->srv.body_bytes is known after it
int mtxw_build(nabo_mtxw *h, const int64_t *cell_ptr, const int32_t *gene, const uint32_t *val, const std::vector<int32_t> &long_list, int64_t budget)
{
    hipStream_t st = nullptr;
    const int64_t n_cells = h->n_cells, nnz = h->nnz, n_long = (int64_t)long_list.size();
    if (budget <= 0) {
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        budget = (int64_t)(free_b / 4 * 3);
    }
    size_t temp = 0;
    HIP_TRY(nabo::scan_u64_temp_bytes(n_cells + 1, &temp));
    const int64_t peak = 12 * nnz + 24 * (n_cells + 1) + 4 * n_long + (h->chunk + 16) + 64 + (int64_t)temp;
    if (peak > budget)
        return nabo::api_fail(NABO_E_NOMEM, "nnz = %lld, n_cells = %lld with chunks of %lld bytes needs %lld bytes of device memory, the budget is %lld",
                              (long long)nnz, (long long)n_cells, (long long)h->chunk, (long long)peak, (long long)budget);
    HIP_TRY(h->d_ptr.alloc((size_t)(n_cells + 1) * 8));
    HIP_TRY(h->d_gene.alloc((size_t)nnz * 4));
    HIP_TRY(h->d_val.alloc((size_t)nnz * 4));
    HIP_TRY(h->d_ent_off.alloc((size_t)nnz * 4));
    HIP_TRY(h->d_len.alloc((size_t)(n_cells + 1) * 8));
    HIP_TRY(h->d_off.alloc((size_t)(n_cells + 1) * 8));
    HIP_TRY(h->d_long.alloc((size_t)n_long * 4));
    HIP_TRY(h->d_temp.alloc(temp));
    HIP_TRY(h->ev.create());
    HIP_TRY(hipEventRecord(h->ev.ev[0], st));
    HIP_TRY(hipMemcpyAsync(h->d_ptr.p, cell_ptr, (size_t)(n_cells + 1) * 8, hipMemcpyHostToDevice, st));
    if (nnz > 0) {
        HIP_TRY(hipMemcpyAsync(h->d_gene.p, gene, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(h->d_val.p, val, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
    }
    if (n_long > 0) HIP_TRY(hipMemcpyAsync(h->d_long.p, long_list.data(), (size_t)n_long * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(h->ev.ev[1], st));
    HIP_TRY(hipMemsetAsync(h->d_len.as<uint64_t>() + n_cells, 0, 8, st));
    if (n_cells > 0)
        hipLaunchKernelGGL(nabo::mtxw_len_kernel, dim3(nabo::groups_grid(n_cells)), dim3(nabo::CW_BLOCK), 0, st, h->d_ptr.as<int64_t>(),
                           h->d_gene.as<int32_t>(), h->d_val.as<uint32_t>(), n_cells, h->blank, h->d_ent_off.as<uint32_t>(), h->d_len.as<uint64_t>());
    if (n_long > 0)
        hipLaunchKernelGGL(nabo::mtxw_len_long_kernel, dim3((unsigned)n_long), dim3(nabo::CW_BLOCK), 0, st, h->d_ptr.as<int64_t>(),
                           h->d_gene.as<int32_t>(), h->d_val.as<uint32_t>(), h->d_long.as<int32_t>(), h->d_ent_off.as<uint32_t>(),
                           h->d_len.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(nabo::scan_u64_launch(h->d_temp.p, h->d_temp.cap, h->d_len.as<uint64_t>(), h->d_off.as<uint64_t>(), n_cells + 1, st));
    HIP_TRY(hipEventRecord(h->ev.ev[2], st));
    uint64_t body = 0;
    HIP_TRY(hipMemcpyAsync(&body, h->d_off.as<uint64_t>() + n_cells, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(h->ev.elapsed(0, 1, &h->ms[0]));
    HIP_TRY(h->ev.elapsed(1, 2, &h->ms[1]));
    h->srv.body_bytes = (int64_t)body;
    h->d_len.release();
    h->d_temp.release();
    const int64_t room = std::min<int64_t>(h->chunk, ((int64_t)body + 15) / 16 * 16);
    HIP_TRY(h->d_text.alloc((size_t)room + 16));
    HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&h->pinned), (size_t)room + 16, hipHostMallocDefault));
    h->srv.chunk = h->pinned;
    return NABO_OK;
}

// formats the body bytes from `at` on into the chunk buffer and brings them to the host
int mtxw_next_chunk(nabo_mtxw *h, int64_t at)
{
    hipStream_t st = nullptr;
    const int64_t len = std::min<int64_t>(h->chunk, h->srv.body_bytes - at);
    const int64_t n_tiles = (len + nabo::CW_TILE - 1) / nabo::CW_TILE;
    HIP_TRY(hipEventRecord(h->ev.ev[0], st));
    hipLaunchKernelGGL(nabo::mtxw_format_kernel, dim3((unsigned)n_tiles), dim3(nabo::CW_BLOCK), 0, st, h->d_ptr.as<int64_t>(), h->d_gene.as<int32_t>(),
                       h->d_val.as<uint32_t>(), h->d_ent_off.as<uint32_t>(), h->d_off.as<uint64_t>(), h->n_cells, h->blank, at, len,
                       h->d_text.as<uint4>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->ev.ev[1], st));
    HIP_TRY(hipMemcpyAsync(h->pinned, h->d_text.p, (size_t)len, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(h->ev.ev[2], st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(h->ev.elapsed(0, 1, &h->ms[2]));
    HIP_TRY(h->ev.elapsed(1, 2, &h->ms[3]));
    h->srv.chunk_at = at;
    h->srv.chunk_len = len;
    ++h->n_chunks;
    return NABO_OK;
}

}  // namespace

extern "C" {

int nabo_mtxw_create(int32_t device, int64_t n_genes, int64_t n_cells, const int64_t *cell_ptr, const int32_t *gene, const uint32_t *val,
                     const char *comments, int32_t blank_line_for_empty_cell, int64_t chunk_bytes, int64_t mem_budget_bytes, nabo_mtxw **out,
                     int64_t *total_bytes)
{
    if (!out) return nabo::api_fail(NABO_E_INVALID, "out is NULL");
    *out = nullptr;
    int rc = size_check("n_genes", n_genes, (int64_t)1 << 31, "2^31");
    if (rc || (rc = size_check("n_cells", n_cells, (int64_t)1 << 31, "2^31"))) return rc;
    if ((rc = nabo::check_csr_ptr("cell_ptr", "cell", n_cells, cell_ptr))) return rc;
    const int64_t nnz = cell_ptr[n_cells];
    if (nnz >= 0xFFFFFFFFll) return nabo::api_fail(NABO_E_UNSUPPORTED, "nnz=%lld must be below 2^32 - 1", (long long)nnz);
    const cnt::IdxVerdict v = cnt::check_indices(n_cells, n_genes, cell_ptr, gene, val);
    if (v.code) return index_fail(v, "cell", "gene", n_genes, gene);
    if (!cnt::comments_ok(comments)) return nabo::api_fail(NABO_E_INVALID, "comments must be whole lines, each starting with '%%' and ending in a newline");
    if ((rc = nabo::use_device(device))) return rc;
    return nabo::create_handle(out, device, "nabo_mtxw_create", [&](nabo_mtxw *h) {
        std::vector<int32_t> long_list;
        const int64_t longest = cnt::long_cells(n_cells, cell_ptr, &long_list);
        if (longest > cnt::MAX_CELL_ENTRIES)
            return nabo::api_fail(NABO_E_UNSUPPORTED, "a cell of %lld entries: at most %lld are supported", (long long)longest, (long long)cnt::MAX_CELL_ENTRIES);
        h->n_cells = n_cells;
        h->nnz = nnz;
        h->blank = blank_line_for_empty_cell != 0;
        h->chunk = cnt::clamp_chunk(chunk_bytes);
        h->srv.head = cnt::head_text(comments, n_genes, n_cells, nnz);
        const int r = mtxw_build(h, cell_ptr, gene, val, long_list, mem_budget_bytes);
        if (r == NABO_OK && total_bytes) *total_bytes = h->srv.total();
        return r;
    });
}

int nabo_mtxw_read(nabo_mtxw *h, void *buf, int64_t cap, int64_t *n)
{
    if (!h || !buf || !n) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    *n = 0;
    if (cap < 1) return nabo::api_fail(NABO_E_INVALID, "cap=%lld must be at least 1", (long long)cap);
    if (h->failed) return nabo::api_fail(NABO_E_INVALID, "the writer has failed before; only nabo_mtxw_free is left");
    int rc = nabo::use_device(h->device);
    if (rc) return rc;
    uint8_t *p = static_cast<uint8_t *>(buf);
    while (*n < cap) {
        if (h->srv.need_chunk() && (rc = mtxw_next_chunk(h, h->srv.body_pos()))) {
            h->failed = true;
            return rc;
        }
        const int64_t took = h->srv.take(p + *n, cap - *n);
        if (took == 0) break;
        *n += took;
    }
    return NABO_OK;
}

int nabo_mtxw_last_device_ms(nabo_mtxw *h, double ms[4], int64_t *n_chunks)
{
    if (!h || !ms) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    for (int i = 0; i < 4; ++i) ms[i] = h->ms[i];
    if (n_chunks) *n_chunks = h->n_chunks;
    return NABO_OK;
}

void nabo_mtxw_free(nabo_mtxw *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    delete h;
}

int nabo_mtxw_geometry(int32_t *tile_bytes, int32_t *min_chunk, int32_t *long_cell, int32_t *max_line)
{
    if (!tile_bytes || !min_chunk || !long_cell || !max_line) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    *tile_bytes = cnt::TILE_BYTES;
    *min_chunk = (int32_t)cnt::MIN_CHUNK;
    *long_cell = cnt::LONG_CELL;
    *max_line = cnt::MAX_LINE;
    return NABO_OK;
}

int nabo_counts_remap(int32_t device, int64_t n_rows, int64_t n_cols, const int64_t *ptr, const int32_t *idx, const uint32_t *val,
                      int64_t n_out_rows, const int64_t *row_src, int64_t n_out_cols, const int32_t *col_map, int64_t *out_nnz,
                      int64_t *out_ptr, int32_t *out_idx, uint32_t *out_val, int64_t *csc_ptr, int32_t *csc_idx, uint32_t *csc_val)
{
    const int64_t lim = ((int64_t)1 << 31) - 1;
    int rc = size_check("n_rows", n_rows, lim, "2^31 - 1");
    if (rc || (rc = size_check("n_cols", n_cols, lim, "2^31 - 1")) || (rc = size_check("n_out_rows", n_out_rows, lim, "2^31 - 1")) ||
        (rc = size_check("n_out_cols", n_out_cols, lim, "2^31 - 1")))
        return rc;
    if ((rc = nabo::check_csr_ptr("ptr", "row", n_rows, ptr))) return rc;
    const cnt::IdxVerdict v = cnt::check_indices(n_rows, n_cols, ptr, idx, val);
    if (v.code) return index_fail(v, "row", "column", n_cols, idx);
    if ((n_out_rows > 0 && !row_src) || (n_cols > 0 && !col_map)) return nabo::api_fail(NABO_E_INVALID, "row_src or col_map is NULL");
    const cnt::RemapPlan plan = cnt::plan_remap(n_rows, n_cols, ptr, n_out_rows, row_src, n_out_cols, col_map);
    if (plan.code == cnt::REMAP_ROW_SRC)
        return nabo::api_fail(NABO_E_INVALID, "row_src[%lld] = %lld is not a row in [0, %lld)", (long long)plan.at, (long long)row_src[plan.at], (long long)n_rows);
    if (plan.code == cnt::REMAP_COL_MAP)
        return nabo::api_fail(NABO_E_INVALID, "col_map[%lld] = %lld is neither -1 nor a column in [0, %lld)", (long long)plan.at, (long long)col_map[plan.at],
                              (long long)n_out_cols);
    const int64_t B = plan.bound, nnz = ptr[n_rows];
    if (B >= 0xFFFFFFFFll) return nabo::api_fail(NABO_E_UNSUPPORTED, "the bound on the entries, %lld, must be below 2^32 - 1", (long long)B);
    const bool want_csc = csc_ptr || csc_idx || csc_val;
    if (!out_nnz || !out_ptr || (B > 0 && (!out_idx || !out_val))) return nabo::api_fail(NABO_E_INVALID, "an output array is NULL");
    if (want_csc && (!csc_ptr || (B > 0 && (!csc_idx || !csc_val))))
        return nabo::api_fail(NABO_E_INVALID, "csc_ptr, csc_idx and csc_val must be given together or all be NULL");
    if ((rc = nabo::use_device(device))) return rc;
    hipStream_t st = nullptr;
    DevBuf d_ptr, d_idx, d_val, d_src, d_map, d_count, d_out_ptr, d_temp, d_dup, key[2], kv[2], d_lo, d_csc_ptr;
    size_t temp = 0;
    HIP_TRY(nabo::scan_u64_temp_bytes(n_out_rows + 1, &temp));
    HIP_TRY(d_ptr.alloc((size_t)(n_rows + 1) * 8));
    HIP_TRY(d_idx.alloc((size_t)nnz * 4));
    HIP_TRY(d_val.alloc((size_t)nnz * 4));
    HIP_TRY(d_src.alloc((size_t)n_out_rows * 8));
    HIP_TRY(d_map.alloc((size_t)n_cols * 4));
    HIP_TRY(d_count.alloc((size_t)(n_out_rows + 1) * 8));
    HIP_TRY(d_out_ptr.alloc((size_t)(n_out_rows + 1) * 8));
    HIP_TRY(d_temp.alloc(temp));
    HIP_TRY(d_dup.alloc(8));
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(key[i].alloc((size_t)B * 8));
        HIP_TRY(kv[i].alloc((size_t)B * 4));
    }
    HIP_TRY(d_lo.alloc((size_t)B * 4));
    HIP_TRY(hipMemcpyAsync(d_ptr.p, ptr, (size_t)(n_rows + 1) * 8, hipMemcpyHostToDevice, st));
    if (nnz > 0) {
        HIP_TRY(hipMemcpyAsync(d_idx.p, idx, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_val.p, val, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
    }
    if (n_out_rows > 0) HIP_TRY(hipMemcpyAsync(d_src.p, row_src, (size_t)n_out_rows * 8, hipMemcpyHostToDevice, st));
    if (n_cols > 0) HIP_TRY(hipMemcpyAsync(d_map.p, col_map, (size_t)n_cols * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_count.as<int64_t>() + n_out_rows, 0, 8, st));
    const unsigned grid = nabo::groups_grid(n_out_rows);
    if (n_out_rows > 0)
        hipLaunchKernelGGL(nabo::remap_count_kernel, dim3(grid), dim3(nabo::CW_BLOCK), 0, st, d_ptr.as<int64_t>(), d_idx.as<int32_t>(), d_src.as<int64_t>(),
                           d_map.as<int32_t>(), n_out_rows, d_count.as<int64_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(nabo::scan_u64_launch(d_temp.p, d_temp.cap, d_count.as<uint64_t>(), d_out_ptr.as<uint64_t>(), n_out_rows + 1, st));
    if (n_out_rows > 0)
        hipLaunchKernelGGL(nabo::remap_write_kernel, dim3(grid), dim3(nabo::CW_BLOCK), 0, st, d_ptr.as<int64_t>(), d_idx.as<int32_t>(), d_val.as<uint32_t>(),
                           d_src.as<int64_t>(), d_map.as<int32_t>(), n_out_rows, d_out_ptr.as<int64_t>(), key[0].as<uint64_t>(), kv[0].as<uint32_t>());
    HIP_TRY(hipGetLastError());
    int64_t n_out = 0;
    HIP_TRY(hipMemcpyAsync(&n_out, d_out_ptr.as<int64_t>() + n_out_rows, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    size_t sort_temp = 0;
    HIP_TRY(nabo::mtx_sort_temp_bytes(n_out, n_out_rows, n_out_cols, &sort_temp));
    HIP_TRY(d_temp.alloc(sort_temp));
    uint64_t *k[2] = {key[0].as<uint64_t>(), key[1].as<uint64_t>()};
    uint32_t *w[2] = {kv[0].as<uint32_t>(), kv[1].as<uint32_t>()};
    int which = 0;
    unsigned long long dup = ~0ull;
    if (!plan.monotone) HIP_TRY(nabo::mtx_sort_launch(k, w, &which, n_out, n_out_rows, n_out_cols, true, d_temp.p, d_temp.cap, st));
    HIP_TRY(nabo::mtx_dup_launch(k[which], n_out, d_dup.as<unsigned long long>(), st));
    HIP_TRY(nabo::mtx_split_launch(k[which], n_out, d_lo.as<uint32_t>(), nullptr, st));
    HIP_TRY(hipMemcpyAsync(&dup, d_dup.p, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (dup != ~0ull)
        return nabo::api_fail(NABO_E_INVALID, "output row %llu holds output column %llu more than once: two kept columns of its source row map to it",
                              dup >> 32, dup & 0xFFFFFFFFull);
    *out_nnz = n_out;
    HIP_TRY(hipMemcpyAsync(out_ptr, d_out_ptr.p, (size_t)(n_out_rows + 1) * 8, hipMemcpyDeviceToHost, st));
    if (n_out > 0) {
        HIP_TRY(hipMemcpyAsync(out_idx, d_lo.p, (size_t)n_out * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_val, w[which], (size_t)n_out * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (!want_csc) return NABO_OK;
    HIP_TRY(d_csc_ptr.alloc((size_t)(n_out_cols + 1) * 8));
    uint32_t *rows = nullptr;
    if ((rc = nabo::mtx_transpose_stage(key, kv, &which, n_out, n_out_rows, n_out_cols, d_temp.p, d_temp.cap, d_csc_ptr.as<int64_t>(), &rows, st))) return rc;
    HIP_TRY(hipMemcpyAsync(csc_ptr, d_csc_ptr.p, (size_t)(n_out_cols + 1) * 8, hipMemcpyDeviceToHost, st));
    if (n_out > 0) {
        HIP_TRY(hipMemcpyAsync(csc_idx, rows, (size_t)n_out * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(csc_val, kv[which].p, (size_t)n_out * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return NABO_OK;
}

}  // extern "C"
