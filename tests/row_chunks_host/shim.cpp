// The row-chunk planner and the gather of a chunk (nabo_amd/csrc/row_chunks.h) compiled for the host alone, callable from
// tests/test_row_chunks_cpu.py.
#include "row_chunks.h"

using namespace nabo;

extern "C" {

// start: room for n_rows + 2 entries; out: max_rows, max_nnz, big_row, big_bytes.  Returns the entries of start.
int64_t rc_plan(int64_t n_rows, const int64_t *rows, const int64_t *cell_ptr, int64_t fixed, int64_t room, int64_t cap, int64_t *start,
                int64_t out[4])
{
    const RowChunks p = plan_row_chunks(n_rows, rows, cell_ptr, fixed, room, cap);
    if (!p.start.empty()) memcpy(start, p.start.data(), p.start.size() * 8);
    out[0] = p.max_rows;
    out[1] = p.max_nnz;
    out[2] = p.big_row;
    out[3] = p.big_bytes;
    return (int64_t)p.start.size();
}

// src: the addresses the entries are to be read from, gene then val.  Returns the chunk's entries.
int64_t rc_gather(int64_t r0, int64_t nr, const int64_t *cell_ptr, const int32_t *gene, const float *val, const float *sf, const int64_t *rows,
                  int64_t *h_ptr, float *h_sf, int32_t *h_gene, float *h_val, const void *src[2])
{
    const RowSlice s = gather_rows(r0, nr, cell_ptr, gene, val, sf, rows, h_ptr, h_sf, h_gene, h_val);
    src[0] = s.gene;
    src[1] = s.val;
    return s.nnz;
}

}  // extern "C"
