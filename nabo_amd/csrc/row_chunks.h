// row_chunks.h -- how the steps that stream rows of cells (per-cell QC, the PCA projection, the PCA fit) cut their rows
// into chunks within a byte budget, and a chunk's rows as one CSR.  Host only, no HIP: tests/test_row_chunks_cpu.py
// compiles this header alone and checks it without a GPU.
//
// Row r of the output is cell rows[r], or cell r when `rows` is NULL (all cells in order); cell c lists the entries
// cell_ptr[c] .. cell_ptr[c + 1] of gene and val.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

namespace nabo {

struct RowChunks {
    std::vector<int64_t> start;            // chunk c holds the rows [start[c], start[c + 1]); the last entry is n_rows
    int64_t max_rows = 0, max_nnz = 0;     // the most rows and the most entries any chunk holds
    int64_t big_row = -1, big_bytes = 0;   // the first row that alone exceeds the room and what it needs; the plan ends there
};

// A row costs fixed + 8 bytes per entry.  A row joins the current chunk unless that takes the chunk past `room` bytes or
// the chunk holds `cap` rows already; then it starts the next one.
inline RowChunks plan_row_chunks(int64_t n_rows, const int64_t *rows, const int64_t *cell_ptr, int64_t fixed, int64_t room, int64_t cap)
{
    RowChunks p;
    p.start.push_back(0);
    int64_t used = 0, nnz = 0;
    for (int64_t r = 0; r < n_rows; ++r) {
        const int64_t c = rows ? rows[r] : r, ne = cell_ptr[c + 1] - cell_ptr[c], b = fixed + 8 * ne, r0 = p.start.back();
        if (b > room) {
            p.big_row = r;
            p.big_bytes = b;
            return p;
        }
        if (r > r0 && (used + b > room || r - r0 >= cap)) {
            p.start.push_back(r);
            used = nnz = 0;
        }
        used += b;
        nnz += ne;
        p.max_rows = r + 1 - p.start.back() > p.max_rows ? r + 1 - p.start.back() : p.max_rows;
        p.max_nnz = nnz > p.max_nnz ? nnz : p.max_nnz;
    }
    p.start.push_back(n_rows);
    return p;
}

// The rows [r0, r0 + nr) as one CSR: h_ptr [nr + 1] from 0, h_sf [nr] the rows' size factors (when sf and h_sf are given),
// and where the entries are.  Without `rows` that is a slice of the caller's arrays and nothing is copied; with `rows`
// the entries are gathered in output order into h_gene and h_val, which hold the chunk's entries.
struct RowSlice {
    int64_t nnz;
    const int32_t *gene;
    const float *val;
};
inline RowSlice gather_rows(int64_t r0, int64_t nr, const int64_t *cell_ptr, const int32_t *gene, const float *val, const float *sf,
                            const int64_t *rows, int64_t *h_ptr, float *h_sf, int32_t *h_gene, float *h_val)
{
    h_ptr[0] = 0;
    if (!rows) {
        const int64_t e0 = cell_ptr[r0];
        for (int64_t r = 0; r < nr; ++r) h_ptr[r + 1] = cell_ptr[r0 + r + 1] - e0;
        if (sf && h_sf && nr) memcpy(h_sf, sf + r0, (size_t)nr * 4);
        return {h_ptr[nr], gene + e0, val + e0};
    }
    int64_t nnz = 0;
    for (int64_t r = 0; r < nr; ++r) {
        const int64_t c = rows[r0 + r], a = cell_ptr[c], ne = cell_ptr[c + 1] - a;
        if (ne) {
            memcpy(h_gene + nnz, gene + a, (size_t)ne * 4);
            memcpy(h_val + nnz, val + a, (size_t)ne * 4);
        }
        nnz += ne;
        h_ptr[r + 1] = nnz;
        if (sf && h_sf) h_sf[r] = sf[c];
    }
    return {nnz, h_gene, h_val};
}

}  // namespace nabo
