// counts_host.h -- the host half of the Matrix Market writer and of the remap (include/nabo_counts.h), without a single
// HIP call: the geometry, the number of decimal digits and the text of one line (shared with the kernels), the text in
// front of the body, the argument checks that visit every entry, the bounds of a remap and the serving of bytes in any
// `cap`.  counts.hip includes it; the tests compile it with a small main (tests/abi_c/counts_host_main.cpp) under the
// address and undefined-behaviour sanitizers.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/nabo_knn.h"

#if defined(__HIPCC__)
#define NABO_COUNTS_HD __host__ __device__ __forceinline__
#else
#define NABO_COUNTS_HD inline
#endif

namespace nabo {
namespace counts {

// TILE_BYTES of text belong to one workgroup of the format kernel; a cell of more than LONG_CELL entries gets a workgroup
// of its own in the length pass; MAX_LINE: "4294967295 2147483647 4294967295\n" has 33 bytes.
constexpr int TILE_BYTES = 8192, LONG_CELL = 1024, MAX_LINE = 33;
constexpr int64_t DEFAULT_CHUNK = (int64_t)64 << 20, MIN_CHUNK = 64, MAX_CHUNK = (int64_t)1 << 30;
// a cell's text is addressed with 32 bits inside the cell
constexpr int64_t MAX_CELL_ENTRIES = (int64_t)0xFFFFFFFFll / MAX_LINE;
constexpr char BANNER[] = "%%MatrixMarket matrix coordinate integer general\n";

// chunk_bytes as the handle uses it: <= 0 the default, clamped to [MIN_CHUNK, MAX_CHUNK], a whole number of 16 bytes
inline int64_t clamp_chunk(int64_t c)
{
    c = c <= 0 ? DEFAULT_CHUNK : c < MIN_CHUNK ? MIN_CHUNK : c > MAX_CHUNK ? MAX_CHUNK : c;
    return (c + 15) / 16 * 16;
}

// the decimal digits of v, 1 .. 10
NABO_COUNTS_HD int digits10(uint32_t v)
{
    return v < 10u ? 1 : v < 100u ? 2 : v < 1000u ? 3 : v < 10000u ? 4 : v < 100000u ? 5 : v < 1000000u ? 6 : v < 10000000u ? 7 : v < 100000000u ? 8 : v < 1000000000u ? 9 : 10;
}

// the bytes of the line of (gene, cell, value), 0-based gene and cell: "%d %d %d\n" of gene + 1, cell + 1, value
NABO_COUNTS_HD int line_bytes(uint32_t gene, uint32_t cell, uint32_t val) { return digits10(gene + 1u) + digits10(cell + 1u) + digits10(val) + 3; }

// writes the digits of v so that the last one stands at end[-1]; returns where the first one stands
template <class Byte> NABO_COUNTS_HD Byte *put_digits(Byte *end, uint32_t v)
{
    do {
        const uint32_t q = v / 10u;
        *--end = (Byte)('0' + (v - q * 10u));
        v = q;
    } while (v);
    return end;
}

// the line of (gene, cell, value) written backwards from its end: the line occupies [end - line_bytes, end)
template <class Byte> NABO_COUNTS_HD void put_line(Byte *end, uint32_t gene, uint32_t cell, uint32_t val)
{
    *--end = (Byte)'\n';
    end = put_digits(end, val);
    *--end = (Byte)' ';
    end = put_digits(end, cell + 1u);
    *--end = (Byte)' ';
    put_digits(end, gene + 1u);
}

// comments: NULL or empty, or whole lines, each starting with '%' and ending in '\n'
inline bool comments_ok(const char *c)
{
    if (!c) return true;
    while (*c) {
        if (*c != '%') return false;
        const char *nl = strchr(c, '\n');
        if (!nl) return false;
        c = nl + 1;
    }
    return true;
}

// the text in front of the body: banner, comments, size line
inline std::string head_text(const char *comments, int64_t n_genes, int64_t n_cells, int64_t nnz)
{
    char size[96];
    snprintf(size, sizeof size, "%lld %lld %lld\n", (long long)n_genes, (long long)n_cells, (long long)nnz);
    return std::string(BANNER) + (comments ? comments : "") + size;
}

// What is wrong with the entries of a compressed sparse matrix whose pointers have passed check_csr_ptr; the index rules
// are those of check_sparse (in range, strictly increasing inside a list), the values are payloads and not looked at.
enum IdxCode { IDX_OK = 0, IDX_NULL = 1, IDX_RANGE = 2, IDX_ORDER = 3 };
struct IdxVerdict {
    int code;
    int64_t major, entry;
};
inline IdxVerdict check_indices(int64_t n_major, int64_t n_minor, const int64_t *ptr, const int32_t *idx, const void *val)
{
    if (ptr[n_major] > 0 && (!idx || !val)) return {IDX_NULL, 0, 0};
    for (int64_t i = 0; i < n_major; ++i) {
        int64_t last = -1;
        for (int64_t e = ptr[i]; e < ptr[i + 1]; ++e) {
            const int64_t j = idx[e];
            if (j < 0 || j >= n_minor) return {IDX_RANGE, i, e};
            if (j <= last) return {IDX_ORDER, i, e};
            last = j;
        }
    }
    return {IDX_OK, 0, 0};
}

// the cells of more than LONG_CELL entries, and the longest cell
inline int64_t long_cells(int64_t n_cells, const int64_t *ptr, std::vector<int32_t> *out)
{
    int64_t longest = 0;
    for (int64_t c = 0; c < n_cells; ++c) {
        const int64_t n = ptr[c + 1] - ptr[c];
        if (n > LONG_CELL) out->push_back((int32_t)c);
        if (n > longest) longest = n;
    }
    return longest;
}

// The bytes of the body on the host, the statement the format kernel is held to: cell by cell, a line per entry, a
// single `\n` for a cell without entries when `blank` is set.
inline std::string body_text(int64_t n_cells, const int64_t *ptr, const int32_t *gene, const uint32_t *val, bool blank)
{
    std::string out;
    char line[MAX_LINE];
    for (int64_t c = 0; c < n_cells; ++c) {
        if (ptr[c] == ptr[c + 1] && blank) out.push_back('\n');
        for (int64_t e = ptr[c]; e < ptr[c + 1]; ++e) {
            const int n = line_bytes((uint32_t)gene[e], (uint32_t)c, val[e]);
            put_line(line + n, (uint32_t)gene[e], (uint32_t)c, val[e]);
            out.append(line, (size_t)n);
        }
    }
    return out;
}

// The arguments of a remap that need no device: the bound B = sum of the lengths of the source rows, and whether col_map
// is non-decreasing over the columns it keeps (then a row's keys come out in order and the sort is skipped).
enum RemapCode { REMAP_OK = 0, REMAP_ROW_SRC = 1, REMAP_COL_MAP = 2 };
struct RemapPlan {
    int code;
    int64_t at, bound;
    bool monotone;
};
inline RemapPlan plan_remap(int64_t n_rows, int64_t n_cols, const int64_t *ptr, int64_t n_out_rows, const int64_t *row_src, int64_t n_out_cols,
                            const int32_t *col_map)
{
    RemapPlan p = {REMAP_OK, 0, 0, true};
    int64_t last = -1;
    for (int64_t j = 0; j < n_cols; ++j) {
        const int64_t m = col_map[j];
        if (m < -1 || m >= n_out_cols) return {REMAP_COL_MAP, j, 0, false};
        if (m < 0) continue;
        if (m < last) p.monotone = false;
        last = m;
    }
    for (int64_t r = 0; r < n_out_rows; ++r) {
        const int64_t s = row_src[r];
        if (s < 0 || s >= n_rows) return {REMAP_ROW_SRC, r, 0, false};
        p.bound += ptr[s + 1] - ptr[s];
    }
    return p;
}

// Serves the text -- the head from host memory, then the body chunk by chunk -- in reads of any cap.  The owner refills
// `chunk` (chunk_len bytes of the body from body_pos on) when need_chunk() says so.
struct Server {
    std::string head;
    int64_t body_bytes = 0, pos = 0;            // pos: bytes of the whole text delivered so far
    const uint8_t *chunk = nullptr;
    int64_t chunk_at = 0, chunk_len = 0;        // the body bytes [chunk_at, chunk_at + chunk_len) are in `chunk`

    int64_t total() const { return (int64_t)head.size() + body_bytes; }
    int64_t body_pos() const { return pos - (int64_t)head.size(); }
    bool need_chunk() const { return pos >= (int64_t)head.size() && pos < total() && body_pos() >= chunk_at + chunk_len; }
    // copies what is at hand, at most cap bytes; 0 at the end or when a chunk is needed first
    int64_t take(uint8_t *buf, int64_t cap)
    {
        int64_t n = 0;
        const int64_t hs = (int64_t)head.size();
        if (pos < hs) {
            n = hs - pos < cap ? hs - pos : cap;
            memcpy(buf, head.data() + pos, (size_t)n);
        } else if (pos < total() && !need_chunk()) {
            const int64_t off = body_pos() - chunk_at, left = chunk_len - off;
            n = left < cap ? left : cap;
            memcpy(buf, chunk + off, (size_t)n);
        }
        pos += n;
        return n;
    }
};

}  // namespace counts
}  // namespace nabo
