// Per-cell quality-control sums (include/nabo_qc.h): the per-cell loops behind Dataset.filter_data and Dataset.set_sf
// (nabo/_dataset.py:208-258, :369-405, :548-592) as ONE streaming pass over the cells' entries.
//
// The kernel reads 8 bytes per entry (gene, val) and one byte of the class table per entry, and adds the value to
// 1 + n_classes float64 accumulators.  GEOMETRY: a cell belongs to a GROUP of 16 lanes, four cells to a wavefront, 32 to
// a workgroup of 512 threads.  A group strides over its cell 16 entries at a time, four strides in flight (64 entries,
// 512 B per group, 2 KiB per wave: what a whole wave striding over one cell would request), so a long cell streams as
// before and a cell of a few entries costs a quarter of a wave, not a whole one; the price is that a wave runs as long
// as the longest of its four cells.  One width serves every cell, so the order of a sum depends on the cell alone --
// never on the chunk it travels in or on its neighbours -- and the header can state it: lane j of the group adds the
// entries e = j, j + 16, ... in turn, a butterfly over 8, 4, 2, 1 combines the 16 lanes, lane 0 writes.  No atomics.
// CLASS TABLE: n_raw_genes bytes.  A workgroup copies it into LDS once (16 bytes per lane and step) when it holds at
// most QC_LDS_TABLE_GENES genes, and then walks over tiles of 32 cells with the grid's stride, so the copy is paid once
// per workgroup and not once per tile; a larger table is read through L2 where it stays resident.  Without classes
// there is no table.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <cmath>
#include <vector>

#include "../../include/nabo_qc.h"
#include "host_common.h"

namespace nabo {

constexpr int QC_GROUP = 16;                            // lanes per cell
constexpr int QC_BLOCK = 512;
constexpr int QC_CELLS_PER_WG = QC_BLOCK / QC_GROUP;    // 32
constexpr int QC_INFLIGHT = 4;                          // strides of 16 entries a group requests before it adds the first
constexpr int QC_LDS_TABLE_GENES = 65536;               // the class table goes to LDS up to this many genes
constexpr int QC_LDS_PER_CU = 160 * 1024;

// ptr: the chunk's row pointers relative to its first entry, [n_rows + 1]; table: the class bytes, padded with zeros to
// table_vec16 * 16 bytes; NC: the accumulators compiled in beside the total (>= n_classes); out_sums: [n_rows, 1 + n_classes]
template <int NC, bool LDS>
__global__ __launch_bounds__(QC_BLOCK) void cell_qc_kernel(const int64_t *__restrict__ ptr, const int32_t *__restrict__ gene,
                                                           const float *__restrict__ val, int64_t n_rows, const uint8_t *__restrict__ table,
                                                           int table_vec16, int n_classes, int64_t *__restrict__ out_n,
                                                           double *__restrict__ out_sums)
{
    extern __shared__ uint4 qc_lds[];
    const uint8_t *cls = table;
    if (NC > 0 && LDS) {
        const uint4 *src = reinterpret_cast<const uint4 *>(table);
        for (int i = threadIdx.x; i < table_vec16; i += QC_BLOCK) qc_lds[i] = src[i];
        __syncthreads();
        cls = reinterpret_cast<const uint8_t *>(qc_lds);
    }
    const int lane = threadIdx.x & (QC_GROUP - 1), grp = threadIdx.x / QC_GROUP;
    const unsigned bits = (1u << n_classes) - 1u;
    const int64_t n_tiles = (n_rows + QC_CELLS_PER_WG - 1) / QC_CELLS_PER_WG;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t r = tile * QC_CELLS_PER_WG + grp;
        const bool live = r < n_rows;                          // a group past the last row walks an empty cell and stores nothing
        const int64_t e0 = live ? ptr[r] : 0, e1 = live ? ptr[r + 1] : 0;
        double acc[NC + 1];
#pragma unroll
        for (int k = 0; k <= NC; ++k) acc[k] = 0.0;
        for (int64_t b = e0; b < e1; b += QC_GROUP * QC_INFLIGHT) {
            int g[QC_INFLIGHT];
            float v[QC_INFLIGHT];
#pragma unroll
            for (int u = 0; u < QC_INFLIGHT; ++u) {
                const int64_t e = b + u * QC_GROUP + lane;
                const int64_t ec = e < e1 ? e : e1 - 1;         // past the end: the last entry again, read and counted as 0.0
                g[u] = gene[ec];
                v[u] = val[ec];
                if (e >= e1) v[u] = 0.0f;
            }
#pragma unroll
            for (int u = 0; u < QC_INFLIGHT; ++u) {
                const double x = (double)v[u];
                acc[0] = acc[0] + x;
                if (NC > 0) {
                    const unsigned c = cls[g[u]] & bits;
#pragma unroll
                    for (int k = 0; k < NC; ++k) acc[1 + k] = acc[1 + k] + (((c >> k) & 1u) ? x : 0.0);
                }
            }
        }
#pragma unroll
        for (int d = QC_GROUP / 2; d > 0; d >>= 1) {
#pragma unroll
            for (int k = 0; k <= NC; ++k) acc[k] = acc[k] + __shfl_xor(acc[k], d, QC_GROUP);
        }
        if (live && lane == 0) {
            out_n[r] = e1 - e0;
            double *o = out_sums + r * (int64_t)(1 + n_classes);
#pragma unroll
            for (int k = 0; k <= NC; ++k)
                if (k <= n_classes) o[k] = acc[k];
        }
    }
}

template <int NC, bool LDS>
static hipError_t cell_qc_launch_as(const int64_t *ptr, const int32_t *gene, const float *val, int64_t n_rows, const uint8_t *table,
                                    int table_vec16, int n_classes, int64_t *out_n, double *out_sums, int cus, hipStream_t st)
{
    const size_t lds = NC > 0 && LDS ? (size_t)table_vec16 * 16 : 0;
    int per_cu = 2048 / QC_BLOCK;                              // the CU's 32 waves
    if (lds && (int)(QC_LDS_PER_CU / lds) < per_cu) per_cu = (int)(QC_LDS_PER_CU / lds);
    const int64_t n_tiles = (n_rows + QC_CELLS_PER_WG - 1) / QC_CELLS_PER_WG, cap = (int64_t)cus * per_cu;
    const dim3 grid((unsigned)(n_tiles < cap ? n_tiles : cap)), block(QC_BLOCK);
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&cell_qc_kernel<NC, LDS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((cell_qc_kernel<NC, LDS>), grid, block, lds, st, ptr, gene, val, n_rows, table, table_vec16, n_classes, out_n, out_sums);
    return hipGetLastError();
}

hipError_t cell_qc_launch(const int64_t *ptr, const int32_t *gene, const float *val, int64_t n_rows, const uint8_t *table,
                          int64_t n_raw_genes, int n_classes, int64_t *out_n, double *out_sums, hipStream_t st)
{
    if (n_rows <= 0) return hipSuccess;
    int dev = 0, cus = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    if (cus < 1) cus = 1;
    const int vec16 = (int)((n_raw_genes + 15) / 16);
    const bool lds = n_raw_genes <= QC_LDS_TABLE_GENES;
#define QC_GO(NC, L) return cell_qc_launch_as<NC, L>(ptr, gene, val, n_rows, table, vec16, n_classes, out_n, out_sums, cus, st)
    if (n_classes == 0) QC_GO(0, false);
    if (n_classes <= 3) {
        if (lds) QC_GO(3, true);
        QC_GO(3, false);
    }
    if (lds) QC_GO(8, true);
    QC_GO(8, false);
#undef QC_GO
}

}  // namespace nabo

// ---- the C ABI --------------------------------------------------------------------------------------------------------
namespace {

using nabo::DevBuf;

constexpr int64_t QC_DEFAULT_BUDGET = (int64_t)2 << 30;
constexpr int64_t QC_MAX_CHUNK_ROWS = (int64_t)1 << 30;

thread_local double g_qc_ms[3] = {0, 0, 0};
thread_local int64_t g_qc_chunks = 0;

}  // namespace

extern "C" {

int nabo_cell_qc(int32_t device, int64_t n_cells, int64_t n_raw_genes, const int64_t *cell_ptr, const int32_t *gene, const float *val,
                 int32_t n_classes, const uint8_t *gene_class, int64_t n_rows, const int64_t *rows, int64_t mem_budget_bytes,
                 int64_t *out_n_entries, double *out_sums)
{
    if (n_cells < 0 || n_cells >= ((int64_t)1 << 31) - 1) return nabo::api_fail(NABO_E_INVALID, "n_cells=%lld out of range [0, 2^31 - 1)", (long long)n_cells);
    if (n_raw_genes < 0 || n_raw_genes >= ((int64_t)1 << 31) - 1) return nabo::api_fail(NABO_E_INVALID, "n_raw_genes=%lld out of range [0, 2^31 - 1)", (long long)n_raw_genes);
    if (n_classes < 0 || n_classes > 8) return nabo::api_fail(NABO_E_INVALID, "n_classes=%d out of range [0, 8]", (int)n_classes);
    if (n_classes > 0 && n_raw_genes > 0 && !gene_class) return nabo::api_fail(NABO_E_INVALID, "gene_class is NULL");
    if (!rows) n_rows = n_cells;
    if (n_rows < 0) return nabo::api_fail(NABO_E_INVALID, "n_rows=%lld is negative", (long long)n_rows);
    if (n_rows > 0 && (!out_n_entries || !out_sums)) return nabo::api_fail(NABO_E_INVALID, "an output array is NULL");
    int rc = nabo::check_sparse<nabo::SPARSE_RAW>(nullptr, "cell", "gene", n_cells, n_raw_genes, cell_ptr, gene, val, nullptr, true);
    if (rc) return rc;
    if ((rc = nabo::check_rows(n_rows, rows, n_cells))) return rc;
    // chunks of rows within the budget
    const int NS = 1 + n_classes;
    const int64_t budget = mem_budget_bytes > 0 ? mem_budget_bytes : QC_DEFAULT_BUDGET;
    const nabo::RowChunks plan = nabo::plan_row_chunks(n_rows, rows, cell_ptr, 16 + 8 * (int64_t)NS, budget, QC_MAX_CHUNK_ROWS);
    if (plan.big_row >= 0)
        return nabo::api_fail(NABO_E_NOMEM, "row %lld alone needs %lld bytes of device buffers, the budget is %lld", (long long)plan.big_row,
                              (long long)plan.big_bytes, (long long)budget);
    const int64_t max_rows = plan.max_rows;
    g_qc_ms[0] = g_qc_ms[1] = g_qc_ms[2] = 0;
    g_qc_chunks = 0;
    if ((rc = nabo::use_device(device))) return rc;
    if (n_rows == 0) return NABO_OK;

    hipStream_t st = nullptr;
    nabo::Events<4> E;
    HIP_TRY(E.create());
    // the class table, padded with zeros to whole 16-byte pieces
    const size_t table_bytes = (size_t)((n_raw_genes + 15) / 16) * 16;
    DevBuf d_table, d_n, d_sums;
    nabo::RowChunk chunk{cell_ptr, gene, val, nullptr, rows};
    HIP_TRY(d_table.alloc(table_bytes));
    if ((rc = chunk.reserve(max_rows, plan.max_nnz))) return rc;
    HIP_TRY(d_n.alloc((size_t)max_rows * 8));
    HIP_TRY(d_sums.alloc((size_t)max_rows * NS * 8));
    if (n_classes > 0 && n_raw_genes > 0) {
        std::vector<uint8_t> h_table(table_bytes, 0);
        memcpy(h_table.data(), gene_class, (size_t)n_raw_genes);
        HIP_TRY(hipEventRecord(E.ev[0], st));
        HIP_TRY(hipMemcpyAsync(d_table.p, h_table.data(), table_bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipEventRecord(E.ev[1], st));
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(E.elapsed(0, 1, &g_qc_ms[0]));
    }
    for (size_t ch = 0; ch + 1 < plan.start.size(); ++ch) {
        const int64_t r0 = plan.start[ch], nr = plan.start[ch + 1] - r0;
        if (nr == 0) continue;
        if ((rc = chunk.upload(r0, nr, st, E.ev[0]))) return rc;
        HIP_TRY(hipEventRecord(E.ev[1], st));
        HIP_TRY(nabo::cell_qc_launch(chunk.d_ptr.as<int64_t>(), chunk.d_gene.as<int32_t>(), chunk.d_val.as<float>(), nr, d_table.as<uint8_t>(),
                                     n_raw_genes, n_classes, d_n.as<int64_t>(), d_sums.as<double>(), st));
        HIP_TRY(hipEventRecord(E.ev[2], st));
        HIP_TRY(hipMemcpyAsync(out_n_entries + r0, d_n.p, (size_t)nr * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_sums + r0 * NS, d_sums.p, (size_t)nr * NS * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipEventRecord(E.ev[3], st));
        HIP_TRY(hipStreamSynchronize(st));
        for (int i = 0; i < 3; ++i) HIP_TRY(E.elapsed(i, i + 1, &g_qc_ms[i]));
        ++g_qc_chunks;
    }
    return NABO_OK;
}

int nabo_qc_last_device_ms(double ms[3], int64_t *n_chunks)
{
    if (!ms) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    for (int i = 0; i < 3; ++i) ms[i] = g_qc_ms[i];
    if (n_chunks) *n_chunks = g_qc_chunks;
    return NABO_OK;
}

}  // extern "C"
