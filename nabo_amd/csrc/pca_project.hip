// PCA projection of sparse cells and per-gene statistics (include/nabo_pca.h): the per-cell loop of
// Dataset.transform_pca (nabo/_dataset.py:985-1033, get_scaled_values :846-915) and the per-gene loop of set_gene_stats
// (:594-637).
//
// PROJECTION.  A cell lists some 5 % of the raw genes and a tenth of those are selected, so the dense scaled vector the
// reference builds per cell is almost all (0 - mu) / sigma: that part is the same for every cell and is folded into one
// bias per component.  What is left per cell is one row of the TRANSPOSED component table [G, C] per listed selected
// gene -- 8 C contiguous bytes, 1.6 MB for 2 000 genes x 100 components, resident in an XCD's L2 -- scaled by
// x / sigma and added in stored order.  One wavefront owns one row of Z: its lanes are the components (lane l holds
// components l, l + 64, ...), it reads 64 entries at a time, computes (gene_pos, x / sigma) once per entry in the lane
// that loaded it and broadcasts the pair; the entries of unselected genes are dropped by a ballot, which keeps the
// stored order.  A row's sum is never split across lanes or waves and there are no atomics, so Z is the header's
// sequential definition bit for bit; the parallelism is the rows.
//
// GENE STATISTICS.  One wavefront per gene column, two passes over the kept cells' entries (sum and count, then the
// squared deviations from the mean), float64 shuffles to reduce.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <cmath>
#include <vector>

#include "../../include/nabo_pca.h"
#include "host_common.h"

namespace nabo {

constexpr int PCA_WAVE = 64;
constexpr int PCA_ROWS_PER_WG = 4;      // one wave per row, 256 threads
constexpr int PCA_INFLIGHT = 4;         // table rows a wave requests before it adds the first

__device__ __forceinline__ int pca_bcast(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ double pca_bcast(double v, int lane)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}

// ptr: the chunk's row pointers relative to its first entry, [n_rows + 1]; sf_row: the size factor of each row's cell;
// Tt: components transposed, [G, C]; Z: [n_rows, C].  CPL: components per lane and pass (a pass covers 64 * CPL).
template <int CPL>
__global__ __launch_bounds__(PCA_WAVE * PCA_ROWS_PER_WG) void pca_project_kernel(
    const int64_t *__restrict__ ptr, const int32_t *__restrict__ gene, const float *__restrict__ val, const float *__restrict__ sf_row,
    int64_t n_rows, const int32_t *__restrict__ gene_pos, const double *__restrict__ sigma, const double *__restrict__ bias,
    const double *__restrict__ Tt, int C, double *__restrict__ Z)
{
    const int lane = threadIdx.x & (PCA_WAVE - 1);
    const int64_t r = (int64_t)blockIdx.x * PCA_ROWS_PER_WG + __builtin_amdgcn_readfirstlane(threadIdx.x / PCA_WAVE);
    if (r >= n_rows) return;
    const int64_t e0 = ptr[r], e1 = ptr[r + 1];
    const float sf = sf_row[r];
    for (int cb = 0; cb < C; cb += PCA_WAVE * CPL) {
        double acc[CPL];
        int col[CPL];
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            const int c = cb + k * PCA_WAVE + lane;
            col[k] = c < C ? c : C - 1;                       // a lane past the last component reads the last one and stores nothing
            acc[k] = bias[col[k]];
        }
        for (int64_t e = e0; e < e1; e += PCA_WAVE) {
            int p = -1;
            double s = 0.0;
            if (e + lane < e1) {
                p = gene_pos[gene[e + lane]];
                if (p >= 0) s = (double)(val[e + lane] * sf) / sigma[p];      // one float32 product, as the reference's `a * self.sf[i]`
            }
            unsigned long long live = __ballot(p >= 0);
            while (live) {
                // up to PCA_INFLIGHT selected entries, in stored order: request their table rows, then add one by one
                int pj[PCA_INFLIGHT];
                double sj[PCA_INFLIGHT], t[PCA_INFLIGHT][CPL];
                const int n = __popcll(live) < PCA_INFLIGHT ? __popcll(live) : PCA_INFLIGHT;
                unsigned long long rest = live;
#pragma unroll
                for (int i = 0; i < PCA_INFLIGHT; ++i) {
                    const int j = rest ? __builtin_ctzll(rest) : __builtin_ctzll(live);   // past the end: the first one again, read and dropped
                    rest &= rest - 1;
                    pj[i] = pca_bcast(p, j);
                    sj[i] = pca_bcast(s, j);
                    const double *row = Tt + (int64_t)pj[i] * C;
#pragma unroll
                    for (int k = 0; k < CPL; ++k) t[i][k] = row[col[k]];
                }
#pragma unroll
                for (int i = 0; i < PCA_INFLIGHT; ++i)
                    if (i < n) {
#pragma unroll
                        for (int k = 0; k < CPL; ++k) acc[k] = acc[k] + sj[i] * t[i][k];
                    }
                live = rest;
            }
        }
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            const int c = cb + k * PCA_WAVE + lane;
            if (c < C) Z[r * C + c] = acc[k];
        }
    }
}

hipError_t pca_project_launch(const int64_t *ptr, const int32_t *gene, const float *val, const float *sf_row, int64_t n_rows,
                              const int32_t *gene_pos, const double *sigma, const double *bias, const double *Tt, int C, double *Z,
                              hipStream_t st)
{
    if (n_rows <= 0 || C <= 0) return hipSuccess;
    const dim3 grid((unsigned)((n_rows + PCA_ROWS_PER_WG - 1) / PCA_ROWS_PER_WG)), block(PCA_WAVE * PCA_ROWS_PER_WG);
    if (C <= PCA_WAVE)
        hipLaunchKernelGGL(pca_project_kernel<1>, grid, block, 0, st, ptr, gene, val, sf_row, n_rows, gene_pos, sigma, bias, Tt, C, Z);
    else if (C <= 2 * PCA_WAVE)
        hipLaunchKernelGGL(pca_project_kernel<2>, grid, block, 0, st, ptr, gene, val, sf_row, n_rows, gene_pos, sigma, bias, Tt, C, Z);
    else
        hipLaunchKernelGGL(pca_project_kernel<4>, grid, block, 0, st, ptr, gene, val, sf_row, n_rows, gene_pos, sigma, bias, Tt, C, Z);
    return hipGetLastError();
}

__device__ __forceinline__ double pca_wave_sum(double v)
{
#pragma unroll
    for (int d = PCA_WAVE / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, PCA_WAVE);
    return v;
}

// gptr: the chunk's column pointers relative to its first entry, [n_genes + 1]; kept: per cell, 1 when it counts;
// keep_gene: per gene of the chunk or NULL; n: the number of kept cells
__global__ __launch_bounds__(PCA_WAVE * PCA_ROWS_PER_WG) void gene_stats_kernel(
    const int64_t *__restrict__ gptr, const int32_t *__restrict__ cell, const float *__restrict__ val, const float *__restrict__ sf,
    const uint8_t *__restrict__ kept, const uint8_t *__restrict__ keep_gene, int64_t n_genes, int64_t n, int64_t *__restrict__ out_ncells,
    uint8_t *__restrict__ out_valid, double *__restrict__ out_m, double *__restrict__ out_nzm, double *__restrict__ out_var)
{
    const int lane = threadIdx.x & (PCA_WAVE - 1);
    const int64_t g = (int64_t)blockIdx.x * PCA_ROWS_PER_WG + __builtin_amdgcn_readfirstlane(threadIdx.x / PCA_WAVE);
    if (g >= n_genes) return;
    int64_t ncells = 0, listed = 0;
    double m = 0.0, nzm = 0.0, var = 0.0;
    if (!keep_gene || keep_gene[g]) {
        const int64_t e0 = gptr[g], e1 = gptr[g + 1];
        double sum = 0.0;
        int pos = 0, cnt = 0;
        for (int64_t e = e0 + lane; e < e1; e += PCA_WAVE) {
            const int32_t c = cell[e];
            if (!kept[c]) continue;
            const float x = val[e] * sf[c];
            sum += (double)x;                                  // x >= 0: the sum of the x > 0 is the sum of all
            pos += x > 0.0f;
            ++cnt;
        }
        sum = pca_wave_sum(sum);
#pragma unroll
        for (int d = PCA_WAVE / 2; d > 0; d >>= 1) {
            pos += __shfl_xor(pos, d, PCA_WAVE);
            cnt += __shfl_xor(cnt, d, PCA_WAVE);
        }
        ncells = pos;
        listed = cnt;
        if (ncells > 0) {
            m = sum / (double)n;
            nzm = sum / (double)ncells;
            double sq = 0.0;
            for (int64_t e = e0 + lane; e < e1; e += PCA_WAVE) {
                const int32_t c = cell[e];
                if (!kept[c]) continue;
                const double dlt = (double)(val[e] * sf[c]) - m;
                sq += dlt * dlt;
            }
            sq = pca_wave_sum(sq);
            var = (sq + (double)(n - listed) * (m * m)) / (double)n;
        }
    }
    if (lane == 0) {
        out_ncells[g] = ncells > 0 ? ncells : 0;
        out_valid[g] = ncells > 0;
        out_m[g] = m;
        out_nzm[g] = nzm;
        out_var[g] = var;
    }
}

hipError_t gene_stats_launch(const int64_t *gptr, const int32_t *cell, const float *val, const float *sf, const uint8_t *kept,
                             const uint8_t *keep_gene, int64_t n_genes, int64_t n_keep, int64_t *out_ncells, uint8_t *out_valid,
                             double *out_m, double *out_nzm, double *out_var, hipStream_t st)
{
    if (n_genes <= 0) return hipSuccess;
    const dim3 grid((unsigned)((n_genes + PCA_ROWS_PER_WG - 1) / PCA_ROWS_PER_WG)), block(PCA_WAVE * PCA_ROWS_PER_WG);
    hipLaunchKernelGGL(gene_stats_kernel, grid, block, 0, st, gptr, cell, val, sf, kept, keep_gene, n_genes, n_keep, out_ncells, out_valid,
                       out_m, out_nzm, out_var);
    return hipGetLastError();
}

// gene_pos, sigma and rows of the projection and of the fit
int pca_check_selection(int64_t n_raw_genes, const int32_t *gene_pos, int64_t G, const double *sigma, int64_t n_cells, int64_t n_rows,
                        const int64_t *rows)
{
    std::vector<uint8_t> seen((size_t)G, 0);
    for (int64_t j = 0; j < n_raw_genes; ++j) {
        const int64_t p = gene_pos[j];
        if (p < -1 || p >= G) return api_fail(NABO_E_INVALID, "gene_pos[%lld] = %lld is neither -1 nor a position in [0, %lld)", (long long)j, (long long)p, (long long)G);
        if (p >= 0 && seen[p]) return api_fail(NABO_E_INVALID, "gene_pos[%lld] = %lld: another raw gene has this position already", (long long)j, (long long)p);
        if (p >= 0) seen[p] = 1;
    }
    for (int64_t p = 0; p < G; ++p)
        if (!(sigma[p] > 0.0) || std::isinf(sigma[p]))
            return api_fail(NABO_E_INVALID, "sigma[%lld] = %g: must be finite and > 0", (long long)p, sigma[p]);
    return check_rows(n_rows, rows, n_cells);
}

}  // namespace nabo

// ---- the C ABI --------------------------------------------------------------------------------------------------------
namespace {

using nabo::DevBuf;

constexpr int64_t PCA_DEFAULT_BUDGET = (int64_t)2 << 30;
constexpr int64_t PCA_MAX_CHUNK_ITEMS = (int64_t)1 << 30;      // rows (genes) of one chunk: the kernels' grids

thread_local double g_pca_ms[3] = {0, 0, 0};
thread_local int64_t g_pca_chunks = 0;

}  // namespace

namespace nabo {
void pca_set_device_ms(const double ms[3], int64_t n_chunks)
{
    for (int i = 0; i < 3; ++i) g_pca_ms[i] = ms[i];
    g_pca_chunks = n_chunks;
}
}  // namespace nabo

extern "C" {

int nabo_pca_project(int32_t device, int64_t n_cells, int64_t n_raw_genes, const int64_t *cell_ptr, const int32_t *gene, const float *val,
                     const float *sf, const int32_t *gene_pos, int64_t n_sel_genes, const double *mu, const double *sigma, const double *mean,
                     int32_t n_comps, const double *components, int64_t n_rows, const int64_t *rows, int64_t mem_budget_bytes, double *out_z)
{
    const int64_t G = n_sel_genes;
    const int C = n_comps;
    if (n_cells < 0 || n_cells >= ((int64_t)1 << 31) - 1) return nabo::api_fail(NABO_E_INVALID, "n_cells=%lld out of range [0, 2^31 - 1)", (long long)n_cells);
    if (n_raw_genes < 0 || n_raw_genes >= ((int64_t)1 << 31) - 1) return nabo::api_fail(NABO_E_INVALID, "n_raw_genes=%lld out of range [0, 2^31 - 1)", (long long)n_raw_genes);
    if (G < 1 || G >= ((int64_t)1 << 31) - 1) return nabo::api_fail(NABO_E_INVALID, "n_sel_genes=%lld out of range [1, 2^31 - 1)", (long long)G);
    if (C < 1 || C > (1 << 20)) return nabo::api_fail(NABO_E_INVALID, "n_comps=%d out of range [1, 2^20]", C);
    if (!mu || !sigma || !mean || !components) return nabo::api_fail(NABO_E_INVALID, "mu, sigma, mean or components is NULL");
    if (n_raw_genes > 0 && !gene_pos) return nabo::api_fail(NABO_E_INVALID, "gene_pos is NULL");
    if (!rows) n_rows = n_cells;
    if (n_rows < 0) return nabo::api_fail(NABO_E_INVALID, "n_rows=%lld is negative", (long long)n_rows);
    if (n_rows > 0 && !out_z) return nabo::api_fail(NABO_E_INVALID, "the output array is NULL");
    int rc = nabo::check_sparse<nabo::SPARSE_RAW_AND_SCALED>(nullptr, "cell", "gene", n_cells, n_raw_genes, cell_ptr, gene, val, sf, true);
    if (rc) return rc;
    if ((rc = nabo::pca_check_selection(n_raw_genes, gene_pos, G, sigma, n_cells, n_rows, rows))) return rc;
    for (int64_t p = 0; p < G; ++p)
        if (!std::isfinite(mu[p]) || !std::isfinite(mean[p]))
            return nabo::api_fail(NABO_E_INVALID, "mu[%lld] = %g, mean[%lld] = %g: must be finite", (long long)p, mu[p], (long long)p, mean[p]);
    for (int64_t i = 0; i < (int64_t)C * G; ++i)
        if (!std::isfinite(components[i]))
            return nabo::api_fail(NABO_E_INVALID, "components[%lld][%lld] = %g: must be finite", (long long)(i / G), (long long)(i % G), components[i]);
    // chunks of rows within the budget
    const int64_t budget = mem_budget_bytes > 0 ? mem_budget_bytes : PCA_DEFAULT_BUDGET;
    const nabo::RowChunks plan = nabo::plan_row_chunks(n_rows, rows, cell_ptr, 12 + 8 * (int64_t)C, budget, PCA_MAX_CHUNK_ITEMS);
    if (plan.big_row >= 0)
        return nabo::api_fail(NABO_E_NOMEM, "row %lld alone needs %lld bytes of device buffers, the budget is %lld", (long long)plan.big_row,
                              (long long)plan.big_bytes, (long long)budget);
    const int64_t max_rows = plan.max_rows;
    g_pca_ms[0] = g_pca_ms[1] = g_pca_ms[2] = 0;
    g_pca_chunks = 0;
    if ((rc = nabo::use_device(device))) return rc;
    if (n_rows == 0) return NABO_OK;

    // the per-gene tables: bias, and the components transposed to [G, C]
    std::vector<double> bias((size_t)C), tt((size_t)G * C);
    for (int c = 0; c < C; ++c) {
        const double *row = components + (int64_t)c * G;
        double acc = 0.0;
        for (int64_t p = 0; p < G; ++p) {
            const double a = (0.0 - mu[p]) / sigma[p], b = a - mean[p], t = b * row[p];
            acc = acc + t;
            tt[(size_t)p * C + c] = row[p];
        }
        bias[c] = acc;
    }
    hipStream_t st = nullptr;
    nabo::Events<4> E;
    HIP_TRY(E.create());
    DevBuf d_pos, d_sigma, d_bias, d_tt, d_z;
    nabo::RowChunk chunk{cell_ptr, gene, val, sf, rows};
    HIP_TRY(d_pos.alloc((size_t)n_raw_genes * 4));
    HIP_TRY(d_sigma.alloc((size_t)G * 8));
    HIP_TRY(d_bias.alloc((size_t)C * 8));
    HIP_TRY(d_tt.alloc((size_t)G * C * 8));
    if ((rc = chunk.reserve(max_rows, plan.max_nnz))) return rc;
    HIP_TRY(d_z.alloc((size_t)max_rows * C * 8));
    HIP_TRY(hipEventRecord(E.ev[0], st));
    if (n_raw_genes) HIP_TRY(hipMemcpyAsync(d_pos.p, gene_pos, (size_t)n_raw_genes * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_sigma.p, sigma, (size_t)G * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_bias.p, bias.data(), (size_t)C * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_tt.p, tt.data(), (size_t)G * C * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(E.ev[1], st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(E.elapsed(0, 1, &g_pca_ms[0]));
    for (size_t ch = 0; ch + 1 < plan.start.size(); ++ch) {
        const int64_t r0 = plan.start[ch], nr = plan.start[ch + 1] - r0;
        if (nr == 0) continue;
        if ((rc = chunk.upload(r0, nr, st, E.ev[0]))) return rc;
        HIP_TRY(hipEventRecord(E.ev[1], st));
        HIP_TRY(nabo::pca_project_launch(chunk.d_ptr.as<int64_t>(), chunk.d_gene.as<int32_t>(), chunk.d_val.as<float>(), chunk.d_sf.as<float>(), nr,
                                         d_pos.as<int32_t>(), d_sigma.as<double>(), d_bias.as<double>(), d_tt.as<double>(), C, d_z.as<double>(), st));
        HIP_TRY(hipEventRecord(E.ev[2], st));
        HIP_TRY(hipMemcpyAsync(out_z + r0 * C, d_z.p, (size_t)nr * C * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipEventRecord(E.ev[3], st));
        HIP_TRY(hipStreamSynchronize(st));
        for (int i = 0; i < 3; ++i) HIP_TRY(E.elapsed(i, i + 1, &g_pca_ms[i]));
        ++g_pca_chunks;
    }
    return NABO_OK;
}

int nabo_gene_stats(int32_t device, int64_t n_genes, int64_t n_cells, const int64_t *gene_ptr, const int32_t *cell, const float *val,
                    const float *sf, int64_t n_keep, const int64_t *keep_cells, const uint8_t *keep_genes, int64_t *out_ncells,
                    uint8_t *out_valid, double *out_m, double *out_nzm, double *out_variance)
{
    if (n_genes < 0 || n_genes >= ((int64_t)1 << 31) - 1) return nabo::api_fail(NABO_E_INVALID, "n_genes=%lld out of range [0, 2^31 - 1)", (long long)n_genes);
    if (n_cells < 0 || n_cells >= ((int64_t)1 << 31) - 1) return nabo::api_fail(NABO_E_INVALID, "n_cells=%lld out of range [0, 2^31 - 1)", (long long)n_cells);
    if (n_genes > 0 && (!out_ncells || !out_valid || !out_m || !out_nzm || !out_variance)) return nabo::api_fail(NABO_E_INVALID, "an output array is NULL");
    int rc = nabo::check_sparse<nabo::SPARSE_RAW_AND_SCALED>(nullptr, "gene", "cell", n_genes, n_cells, gene_ptr, cell, val, sf, false);
    if (rc) return rc;
    std::vector<uint8_t> kept((size_t)n_cells, keep_cells ? 0 : 1);
    if (!keep_cells) n_keep = n_cells;
    if (n_keep < 0) return nabo::api_fail(NABO_E_INVALID, "n_keep=%lld is negative", (long long)n_keep);
    for (int64_t i = 0; keep_cells && i < n_keep; ++i) {
        const int64_t c = keep_cells[i];
        if (c < 0 || c >= n_cells) return nabo::api_fail(NABO_E_INVALID, "keep_cells[%lld] = %lld is not a cell in [0, %lld)", (long long)i, (long long)c, (long long)n_cells);
        if (kept[c]) return nabo::api_fail(NABO_E_INVALID, "keep_cells[%lld] = %lld: the cell is listed twice", (long long)i, (long long)c);
        kept[c] = 1;
    }
    if (n_keep == 0) return nabo::api_fail(NABO_E_INVALID, "no cell is kept: the statistics are means over the kept cells");
    // chunks of genes: 8 bytes per entry within the default budget
    std::vector<int64_t> chunk_start{0};
    int64_t max_genes = 0, max_nnz = 0;
    for (int64_t g = 0; g < n_genes; ++g) {
        const int64_t g0 = chunk_start.back();
        if (g > g0 && ((gene_ptr[g + 1] - gene_ptr[g0]) * 8 > PCA_DEFAULT_BUDGET || g - g0 >= PCA_MAX_CHUNK_ITEMS)) chunk_start.push_back(g);
        const int64_t ng = g + 1 - chunk_start.back(), nz = gene_ptr[g + 1] - gene_ptr[chunk_start.back()];
        max_genes = ng > max_genes ? ng : max_genes;
        max_nnz = nz > max_nnz ? nz : max_nnz;
    }
    chunk_start.push_back(n_genes);
    g_pca_ms[0] = g_pca_ms[1] = g_pca_ms[2] = 0;
    g_pca_chunks = 0;
    if ((rc = nabo::use_device(device))) return rc;
    if (n_genes == 0) return NABO_OK;

    hipStream_t st = nullptr;
    nabo::Events<2> E;
    HIP_TRY(E.create());
    DevBuf d_sf, d_kept, d_keepg, d_gptr, d_cell, d_val, d_nc, d_valid, d_m, d_nzm, d_var;
    HIP_TRY(d_sf.alloc((size_t)n_cells * 4));
    HIP_TRY(d_kept.alloc((size_t)n_cells));
    HIP_TRY(d_keepg.alloc((size_t)max_genes));
    HIP_TRY(d_gptr.alloc((size_t)(max_genes + 1) * 8));
    HIP_TRY(d_cell.alloc((size_t)max_nnz * 4));
    HIP_TRY(d_val.alloc((size_t)max_nnz * 4));
    HIP_TRY(d_nc.alloc((size_t)max_genes * 8));
    HIP_TRY(d_valid.alloc((size_t)max_genes));
    HIP_TRY(d_m.alloc((size_t)max_genes * 8));
    HIP_TRY(d_nzm.alloc((size_t)max_genes * 8));
    HIP_TRY(d_var.alloc((size_t)max_genes * 8));
    if (n_cells) {
        HIP_TRY(hipMemcpyAsync(d_sf.p, sf, (size_t)n_cells * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_kept.p, kept.data(), (size_t)n_cells, hipMemcpyHostToDevice, st));
    }
    std::vector<int64_t> h_gptr((size_t)max_genes + 1);
    for (size_t ch = 0; ch + 1 < chunk_start.size(); ++ch) {
        const int64_t g0 = chunk_start[ch], g1 = chunk_start[ch + 1], ng = g1 - g0;
        if (ng == 0) continue;
        const int64_t e0 = gene_ptr[g0], nnz = gene_ptr[g1] - e0;
        for (int64_t g = 0; g <= ng; ++g) h_gptr[g] = gene_ptr[g0 + g] - e0;
        HIP_TRY(hipMemcpyAsync(d_gptr.p, h_gptr.data(), (size_t)(ng + 1) * 8, hipMemcpyHostToDevice, st));
        if (keep_genes) HIP_TRY(hipMemcpyAsync(d_keepg.p, keep_genes + g0, (size_t)ng, hipMemcpyHostToDevice, st));
        if (nnz) {
            HIP_TRY(hipMemcpyAsync(d_cell.p, cell + e0, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(d_val.p, val + e0, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
        }
        HIP_TRY(hipEventRecord(E.ev[0], st));
        HIP_TRY(nabo::gene_stats_launch(d_gptr.as<int64_t>(), d_cell.as<int32_t>(), d_val.as<float>(), d_sf.as<float>(), d_kept.as<uint8_t>(),
                                        keep_genes ? d_keepg.as<uint8_t>() : nullptr, ng, n_keep, d_nc.as<int64_t>(), d_valid.as<uint8_t>(),
                                        d_m.as<double>(), d_nzm.as<double>(), d_var.as<double>(), st));
        HIP_TRY(hipEventRecord(E.ev[1], st));
        HIP_TRY(hipMemcpyAsync(out_ncells + g0, d_nc.p, (size_t)ng * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_valid + g0, d_valid.p, (size_t)ng, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_m + g0, d_m.p, (size_t)ng * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_nzm + g0, d_nzm.p, (size_t)ng * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_variance + g0, d_var.p, (size_t)ng * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(E.elapsed(0, 1, &g_pca_ms[1]));
        ++g_pca_chunks;
    }
    return NABO_OK;
}

int nabo_pca_last_device_ms(double ms[3], int64_t *n_chunks)
{
    if (!ms) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    for (int i = 0; i < 3; ++i) ms[i] = g_pca_ms[i];
    if (n_chunks) *n_chunks = g_pca_chunks;
    return NABO_OK;
}

}  // extern "C"
