// The exact PCA fit's device half (include/nabo_pca_fit.h): mean and sample covariance of the scaled, sparse cells that
// Dataset.fit_ipca (nabo/_dataset.py:917-983) feeds sklearn in batches.  The eigen-solve of the G x G result is host
// work (nabo_amd/_pca.py).
//
// Two passes over the listed rows, each in chunks of rows that fit the budget:
//   1. DENSIFY the chunk's rows y (one wavefront per cell: fill the row with the per-gene constant (0 - mu) / sigma, then
//      overwrite the listed selected genes), COLUMN SUMS of the dense chunk: a thread owns a column over a slice of the
//      rows, the slices' partial sums are added in slice order, the chunks in chunk order.  mean = sums / n.
//   2. DENSIFY again, centred (constant (0 - mu) / sigma - mean; listed genes ((x - mu) / sigma) - mean), then SYRK:
//      Yc^T Yc with v_mfma_f64_16x16x4_f64 on the 128 x 128 tiles on and below the diagonal.  Lane l of the instruction
//      supplies A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; for Yc^T Yc both are "cell k0 + (l >> 4), gene
//      i0 + (l & 15)" of the same row-major chunk, so a fragment is one LDS read per lane and nothing is transposed.  Its
//      four results per lane sit at col = l & 15, row = (l >> 4) + 4 * reg (NOT the f32 map).  A workgroup of four waves
//      owns one tile, each wave a 64 x 64 quarter as 4 x 4 accumulators; panels of 16 cells x 128 genes go through LDS,
//      the next panel is in flight in registers while the current one is multiplied.  The cell range is split across
//      workgroups; a second kernel adds the partial tiles in split order to the resident accumulator.
// No floating-point atomics: the same call gives the same bits.  The mirror comes from the lower triangle alone.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <cmath>
#include <vector>

#include "../../include/nabo_pca_fit.h"
#include "host_common.h"

namespace nabo {

constexpr int FIT_WAVE = 64;
constexpr int FIT_THREADS = 256;
constexpr int FIT_TILE = 128;                     // genes x genes of one workgroup's output tile
constexpr int FIT_KB = 16;                        // cells per LDS stage
constexpr int FIT_STRIDE = FIT_TILE + 16;         // doubles per LDS row: rows k and k + 1 of a fragment read disjoint banks
constexpr int FIT_MAX_SPLIT = 16;                 // workgroups one tile's cell range is split across, at most
constexpr int FIT_SUM_SPLIT = 256;                // slices of a chunk's rows in the column sums, at most
constexpr int FIT_SUM_ROWS = 64;                  // a slice holds at least this many rows

typedef double fit_d4 __attribute__((ext_vector_type(4)));
typedef double fit_d2 __attribute__((ext_vector_type(2)));

// One wavefront per row of the chunk.  ptr: the chunk's row pointers relative to its first entry; Y: [n_rows_pad, Gp].
// A row is fill[p] (0 in the padding columns p >= G), then ((x - mu) / sigma) - mean at the listed selected genes; the
// padding rows n_rows .. n_rows_pad are 0.
__global__ __launch_bounds__(FIT_THREADS) void pca_densify_kernel(
    const int64_t *__restrict__ ptr, const int32_t *__restrict__ gene, const float *__restrict__ val, const float *__restrict__ sf_row,
    int64_t n_rows, int64_t n_rows_pad, const int32_t *__restrict__ gene_pos, const double *__restrict__ mu, const double *__restrict__ sigma,
    const double *__restrict__ fill, const double *__restrict__ mean, int G, int Gp, double *__restrict__ Y)
{
    const int lane = threadIdx.x & (FIT_WAVE - 1);
    const int64_t r = (int64_t)blockIdx.x * (FIT_THREADS / FIT_WAVE) + __builtin_amdgcn_readfirstlane(threadIdx.x / FIT_WAVE);
    if (r >= n_rows_pad) return;
    double *row = Y + r * Gp;
    if (r >= n_rows) {
        for (int p = lane; p < Gp; p += FIT_WAVE) row[p] = 0.0;
        return;
    }
    for (int p = lane; p < Gp; p += FIT_WAVE) row[p] = p < G ? fill[p] : 0.0;
    __threadfence_block();                         // the constants are written before another lane overwrites one of them
    const int64_t e0 = ptr[r], e1 = ptr[r + 1];
    const float sf = sf_row[r];
    for (int64_t e = e0 + lane; e < e1; e += FIT_WAVE) {
        const int p = gene_pos[gene[e]];
        if (p < 0) continue;
        const double y = ((double)(val[e] * sf) - mu[p]) / sigma[p];      // one float32 product, as the reference's `a * self.sf[i]`
        row[p] = y - mean[p];
    }
}

// partial[slice][p] = the sum of column p over the slice's rows: four threads per column take every fourth row, their
// sums are added in a fixed order
__global__ __launch_bounds__(FIT_THREADS) void pca_colsum_kernel(const double *__restrict__ Y, int64_t n_rows, int Gp, int64_t rows_per_slice,
                                                                 double *__restrict__ partial)
{
    __shared__ double s[FIT_THREADS / FIT_WAVE][FIT_WAVE];
    const int c = threadIdx.x & (FIT_WAVE - 1), sub = threadIdx.x / FIT_WAVE;
    const int col = blockIdx.x * FIT_WAVE + c;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_slice, r1 = r0 + rows_per_slice < n_rows ? r0 + rows_per_slice : n_rows;
    double acc = 0.0;
    if (col < Gp)
        for (int64_t r = r0 + sub; r < r1; r += FIT_THREADS / FIT_WAVE) acc += Y[r * Gp + col];
    s[sub][c] = acc;
    __syncthreads();
    if (sub == 0 && col < Gp) partial[(int64_t)blockIdx.y * Gp + col] = ((s[0][c] + s[1][c]) + s[2][c]) + s[3][c];
}

__global__ __launch_bounds__(FIT_THREADS) void pca_colsum_reduce_kernel(const double *__restrict__ partial, int n_slices, int Gp,
                                                                        double *__restrict__ colsum)
{
    const int col = blockIdx.x * FIT_THREADS + threadIdx.x;
    if (col >= Gp) return;
    double acc = colsum[col];
    for (int s = 0; s < n_slices; ++s) acc += partial[(int64_t)s * Gp + col];
    colsum[col] = acc;
}

// tile t of the lower triangle, row-major: t = ti (ti + 1) / 2 + tj, tj <= ti
__device__ __forceinline__ void fit_tile_of(int64_t t, int &ti, int &tj)
{
    int64_t i = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (i * (i + 1) / 2 > t) --i;
    while ((i + 1) * (i + 2) / 2 <= t) ++i;
    ti = (int)i;
    tj = (int)(t - i * (i + 1) / 2);
}

// a panel is 16 cells x 64 double2; thread t moves double2 number u * 256 + t, u = 0 .. 3, of each of the two panels
constexpr int FIT_PER = FIT_KB * (FIT_TILE / 2) / FIT_THREADS;
__device__ __forceinline__ void fit_fetch(const double *Ai, const double *Bj, int64_t k0, int Gp, int tid, fit_d2 (&ra)[FIT_PER], fit_d2 (&rb)[FIT_PER])
{
#pragma unroll
    for (int u = 0; u < FIT_PER; ++u) {
        const int idx = u * FIT_THREADS + tid, row = idx / (FIT_TILE / 2), col = (idx % (FIT_TILE / 2)) * 2;
        ra[u] = *reinterpret_cast<const fit_d2 *>(Ai + (k0 + row) * Gp + col);
        rb[u] = *reinterpret_cast<const fit_d2 *>(Bj + (k0 + row) * Gp + col);
    }
}

// partial[split][tile][128][128] = sum over the split's cells r of Y[r][ti 128 + i] * Y[r][tj 128 + j].  n_rows_pad and
// rows_per_split are multiples of FIT_KB, Gp of FIT_TILE: every panel read is inside Y.
__global__ __launch_bounds__(FIT_THREADS) void pca_syrk_kernel(const double *__restrict__ Y, int64_t n_rows_pad, int Gp, int64_t rows_per_split,
                                                               int64_t n_tiles, double *__restrict__ partial)
{
    __shared__ __attribute__((aligned(16))) double sA[FIT_KB][FIT_STRIDE];
    __shared__ __attribute__((aligned(16))) double sB[FIT_KB][FIT_STRIDE];
    int ti, tj;
    fit_tile_of(blockIdx.x, ti, tj);
    const int tid = threadIdx.x, lane = tid & (FIT_WAVE - 1), wave = tid / FIT_WAVE;
    const int wi = (wave >> 1) * 64, wj = (wave & 1) * 64;         // the wave's quarter of the tile
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_split;
    const int64_t r1 = r0 + rows_per_split < n_rows_pad ? r0 + rows_per_split : n_rows_pad;
    const double *Ai = Y + (int64_t)ti * FIT_TILE, *Bj = Y + (int64_t)tj * FIT_TILE;
    fit_d4 acc[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = fit_d4{0.0, 0.0, 0.0, 0.0};
    fit_d2 ra[FIT_PER], rb[FIT_PER];
    if (r0 < r1) fit_fetch(Ai, Bj, r0, Gp, tid, ra, rb);
    for (int64_t k0 = r0; k0 < r1; k0 += FIT_KB) {
#pragma unroll
        for (int u = 0; u < FIT_PER; ++u) {
            const int idx = u * FIT_THREADS + tid, row = idx / (FIT_TILE / 2), col = (idx % (FIT_TILE / 2)) * 2;
            *reinterpret_cast<fit_d2 *>(&sA[row][col]) = ra[u];
            *reinterpret_cast<fit_d2 *>(&sB[row][col]) = rb[u];
        }
        __syncthreads();
        if (k0 + FIT_KB < r1) fit_fetch(Ai, Bj, k0 + FIT_KB, Gp, tid, ra, rb);
#pragma unroll
        for (int kk = 0; kk < FIT_KB; kk += 4) {
            double a[4], b[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                a[m] = sA[kk + (lane >> 4)][wi + m * 16 + (lane & 15)];
                b[m] = sB[kk + (lane >> 4)][wj + m * 16 + (lane & 15)];
            }
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n) acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m], b[n], acc[m][n], 0, 0, 0);
        }
        __syncthreads();
    }
    double *out = partial + ((int64_t)blockIdx.y * n_tiles + blockIdx.x) * (FIT_TILE * FIT_TILE);
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int i = wi + m * 16 + (lane >> 4) + 4 * reg, j = wj + n * 16 + (lane & 15);     // the f64 result map
                out[i * FIT_TILE + j] = acc[m][n][reg];
            }
}

// acc[tile][i][j] += partial[0][tile][i][j] + partial[1][tile][i][j] + ..., in split order
__global__ __launch_bounds__(FIT_THREADS) void pca_syrk_reduce_kernel(const double *__restrict__ partial, int n_splits, int64_t n_elems,
                                                                      double *__restrict__ acc)
{
    const int64_t e = (int64_t)blockIdx.x * FIT_THREADS + threadIdx.x;
    if (e >= n_elems) return;
    double a = acc[e];
    for (int s = 0; s < n_splits; ++s) a += partial[(int64_t)s * n_elems + e];
    acc[e] = a;
}

// cov[p][q] = acc(max(p, q), min(p, q)) / (n - 1): both halves from the lower triangle, so the matrix is symmetric bit for bit
__global__ __launch_bounds__(FIT_THREADS) void pca_cov_finish_kernel(const double *__restrict__ acc, int G, double n_minus_1, double *__restrict__ cov)
{
    const int64_t e = (int64_t)blockIdx.x * FIT_THREADS + threadIdx.x;
    if (e >= (int64_t)G * G) return;
    const int p = (int)(e / G), q = (int)(e % G);
    const int hi = p > q ? p : q, lo = p > q ? q : p;
    const int64_t ti = hi / FIT_TILE, tj = lo / FIT_TILE;
    const int64_t t = ti * (ti + 1) / 2 + tj;
    cov[e] = acc[(t * FIT_TILE + hi % FIT_TILE) * FIT_TILE + lo % FIT_TILE] / n_minus_1;
}

int pca_fit_tile() { return FIT_TILE; }
int pca_fit_row_pad() { return FIT_KB; }

int pca_fit_splits(int64_t n_tiles)
{
    // enough workgroups for the device when there are few tiles, one per tile when there are many: a function of G alone
    const int64_t s = (1024 + n_tiles - 1) / n_tiles;
    return (int)(s < 1 ? 1 : s > FIT_MAX_SPLIT ? FIT_MAX_SPLIT : s);
}

int pca_fit_sum_slices() { return FIT_SUM_SPLIT; }

hipError_t pca_densify_launch(const int64_t *ptr, const int32_t *gene, const float *val, const float *sf_row, int64_t n_rows, int64_t n_rows_pad,
                              const int32_t *gene_pos, const double *mu, const double *sigma, const double *fill, const double *mean, int G,
                              int Gp, double *Y, hipStream_t st)
{
    if (n_rows_pad <= 0) return hipSuccess;
    const int per = FIT_THREADS / FIT_WAVE;
    hipLaunchKernelGGL(pca_densify_kernel, dim3((unsigned)((n_rows_pad + per - 1) / per)), dim3(FIT_THREADS), 0, st, ptr, gene, val, sf_row, n_rows,
                       n_rows_pad, gene_pos, mu, sigma, fill, mean, G, Gp, Y);
    return hipGetLastError();
}

// colsum[p] += the sum of column p of Y[n_rows, Gp]; partial: [pca_fit_sum_slices()][Gp]
hipError_t pca_colsum_launch(const double *Y, int64_t n_rows, int Gp, double *partial, double *colsum, hipStream_t st)
{
    if (n_rows <= 0) return hipSuccess;
    int64_t slices = (n_rows + FIT_SUM_ROWS - 1) / FIT_SUM_ROWS;
    if (slices > FIT_SUM_SPLIT) slices = FIT_SUM_SPLIT;
    const int64_t per = (n_rows + slices - 1) / slices;
    slices = (n_rows + per - 1) / per;
    hipLaunchKernelGGL(pca_colsum_kernel, dim3((unsigned)((Gp + FIT_WAVE - 1) / FIT_WAVE), (unsigned)slices), dim3(FIT_THREADS), 0, st, Y, n_rows, Gp,
                       per, partial);
    hipLaunchKernelGGL(pca_colsum_reduce_kernel, dim3((unsigned)((Gp + FIT_THREADS - 1) / FIT_THREADS)), dim3(FIT_THREADS), 0, st, partial,
                       (int)slices, Gp, colsum);
    return hipGetLastError();
}

// acc[n_tiles][128][128] += Y^T Y over the lower-triangle tiles; partial: [pca_fit_splits(n_tiles)][n_tiles][128][128]
hipError_t pca_syrk_launch(const double *Y, int64_t n_rows_pad, int Gp, double *partial, double *acc, hipStream_t st)
{
    if (n_rows_pad <= 0) return hipSuccess;
    const int64_t nT = Gp / FIT_TILE, n_tiles = nT * (nT + 1) / 2, stages = n_rows_pad / FIT_KB;
    int64_t splits = pca_fit_splits(n_tiles);
    if (splits > stages) splits = stages;
    const int64_t per = (stages + splits - 1) / splits;
    splits = (stages + per - 1) / per;
    hipLaunchKernelGGL(pca_syrk_kernel, dim3((unsigned)n_tiles, (unsigned)splits), dim3(FIT_THREADS), 0, st, Y, n_rows_pad, Gp, per * FIT_KB, n_tiles,
                       partial);
    const int64_t n_elems = n_tiles * FIT_TILE * FIT_TILE;
    hipLaunchKernelGGL(pca_syrk_reduce_kernel, dim3((unsigned)((n_elems + FIT_THREADS - 1) / FIT_THREADS)), dim3(FIT_THREADS), 0, st, partial,
                       (int)splits, n_elems, acc);
    return hipGetLastError();
}

hipError_t pca_cov_finish_launch(const double *acc, int G, int64_t n, double *cov, hipStream_t st)
{
    const int64_t e = (int64_t)G * G;
    hipLaunchKernelGGL(pca_cov_finish_kernel, dim3((unsigned)((e + FIT_THREADS - 1) / FIT_THREADS)), dim3(FIT_THREADS), 0, st, acc, G,
                       (double)(n - 1), cov);
    return hipGetLastError();
}

}  // namespace nabo

// ---- the C ABI --------------------------------------------------------------------------------------------------------
namespace {

using nabo::DevBuf;

constexpr int64_t FIT_DEFAULT_BUDGET = (int64_t)2 << 30;
constexpr int64_t FIT_MAX_CHUNK_ROWS = (int64_t)1 << 30;

thread_local double g_fit_phase_ms[3] = {0, 0, 0};

}  // namespace

extern "C" {

int nabo_pca_cov(int32_t device, int64_t n_cells, int64_t n_raw_genes, const int64_t *cell_ptr, const int32_t *gene, const float *val,
                 const float *sf, const int32_t *gene_pos, int64_t n_sel_genes, const double *mu, const double *sigma, int64_t n_rows,
                 const int64_t *rows, int64_t mem_budget_bytes, double *out_mean, double *out_cov)
{
    const int64_t G = n_sel_genes;
    if (n_cells < 0 || n_cells >= ((int64_t)1 << 31) - 1) return nabo::api_fail(NABO_E_INVALID, "n_cells=%lld out of range [0, 2^31 - 1)", (long long)n_cells);
    if (n_raw_genes < 0 || n_raw_genes >= ((int64_t)1 << 31) - 1) return nabo::api_fail(NABO_E_INVALID, "n_raw_genes=%lld out of range [0, 2^31 - 1)", (long long)n_raw_genes);
    if (G < 1 || G >= ((int64_t)1 << 31) - 1) return nabo::api_fail(NABO_E_INVALID, "n_sel_genes=%lld out of range [1, 2^31 - 1)", (long long)G);
    if (!mu || !sigma) return nabo::api_fail(NABO_E_INVALID, "mu or sigma is NULL");
    if (n_raw_genes > 0 && !gene_pos) return nabo::api_fail(NABO_E_INVALID, "gene_pos is NULL");
    if (!rows) n_rows = n_cells;
    if (n_rows < 2) return nabo::api_fail(NABO_E_INVALID, "n_rows=%lld: a covariance needs at least 2 rows", (long long)n_rows);
    if (!out_mean || !out_cov) return nabo::api_fail(NABO_E_INVALID, "an output array is NULL");
    int rc = nabo::check_sparse<nabo::SPARSE_RAW_AND_SCALED>(nullptr, "cell", "gene", n_cells, n_raw_genes, cell_ptr, gene, val, sf, true);
    if (rc) return rc;
    if ((rc = nabo::pca_check_selection(n_raw_genes, gene_pos, G, sigma, n_cells, n_rows, rows))) return rc;
    for (int64_t p = 0; p < G; ++p)
        if (!std::isfinite(mu[p])) return nabo::api_fail(NABO_E_INVALID, "mu[%lld] = %g: must be finite", (long long)p, mu[p]);

    // what stays resident, and chunks of rows within what is left of the budget
    const int64_t budget = mem_budget_bytes > 0 ? mem_budget_bytes : FIT_DEFAULT_BUDGET;
    const int64_t T = nabo::pca_fit_tile(), nT = (G + T - 1) / T, Gp = nT * T;
    const int64_t n_tiles = nT * (nT + 1) / 2, splits = nabo::pca_fit_splits(n_tiles);
    const double fixed_d = (double)n_tiles * (double)(T * T * 8) * (double)(1 + splits) + (double)Gp * 8.0 * (double)nabo::pca_fit_sum_slices();
    if (fixed_d + (double)(12 + 8 * Gp) > (double)budget)
        return nabo::api_fail(NABO_E_NOMEM, "the accumulator and its partial tiles for %lld genes need %.0f bytes and one row %lld more, the budget is %lld",
                              (long long)G, fixed_d, (long long)(12 + 8 * Gp), (long long)budget);
    const int64_t fixed = (int64_t)fixed_d;        // exact: it is below the budget
    const int64_t PAD = nabo::pca_fit_row_pad();
    const nabo::RowChunks plan = nabo::plan_row_chunks(n_rows, rows, cell_ptr, 12 + 8 * Gp, budget - fixed, FIT_MAX_CHUNK_ROWS);
    if (plan.big_row >= 0)
        return nabo::api_fail(NABO_E_NOMEM, "row %lld alone needs %lld bytes of device buffers beside %lld resident ones, the budget is %lld",
                              (long long)plan.big_row, (long long)plan.big_bytes, (long long)fixed, (long long)budget);
    const size_t n_chunks = plan.start.size() - 1;
    double ms3[3] = {0, 0, 0};
    g_fit_phase_ms[0] = g_fit_phase_ms[1] = g_fit_phase_ms[2] = 0;
    nabo::pca_set_device_ms(ms3, 0);
    if ((rc = nabo::use_device(device))) return rc;

    std::vector<double> fill((size_t)G), mean((size_t)G, 0.0);
    for (int64_t p = 0; p < G; ++p) fill[p] = (0.0 - mu[p]) / sigma[p];
    hipStream_t st = nullptr;
    nabo::Events<4> E;
    HIP_TRY(E.create());
    const int64_t max_pad = (plan.max_rows + PAD - 1) / PAD * PAD;
    DevBuf d_pos, d_mu, d_sigma, d_fill, d_mean, d_colsum, d_sumpart, d_acc, d_part, d_y, d_cov;
    nabo::RowChunk chunk{cell_ptr, gene, val, sf, rows};
    HIP_TRY(d_pos.alloc((size_t)n_raw_genes * 4));
    HIP_TRY(d_mu.alloc((size_t)G * 8));
    HIP_TRY(d_sigma.alloc((size_t)G * 8));
    HIP_TRY(d_fill.alloc((size_t)G * 8));
    HIP_TRY(d_mean.alloc((size_t)G * 8));
    HIP_TRY(d_colsum.alloc((size_t)Gp * 8));
    HIP_TRY(d_sumpart.alloc((size_t)Gp * 8 * nabo::pca_fit_sum_slices()));
    HIP_TRY(d_acc.alloc((size_t)(n_tiles * T * T * 8)));
    HIP_TRY(d_part.alloc((size_t)(n_tiles * T * T * 8 * splits)));
    if ((rc = chunk.reserve(plan.max_rows, plan.max_nnz))) return rc;
    HIP_TRY(d_y.alloc((size_t)(max_pad * Gp * 8)));
    HIP_TRY(d_cov.alloc((size_t)(G * G * 8)));
    HIP_TRY(hipEventRecord(E.ev[0], st));
    if (n_raw_genes) HIP_TRY(hipMemcpyAsync(d_pos.p, gene_pos, (size_t)n_raw_genes * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_mu.p, mu, (size_t)G * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_sigma.p, sigma, (size_t)G * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_fill.p, fill.data(), (size_t)G * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_mean.p, mean.data(), (size_t)G * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_colsum.p, 0, (size_t)Gp * 8, st));
    HIP_TRY(hipMemsetAsync(d_acc.p, 0, (size_t)(n_tiles * T * T * 8), st));
    HIP_TRY(hipEventRecord(E.ev[1], st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(E.elapsed(0, 1, &ms3[0]));

    // pass 0: the column sums of y; pass 1: the centred rows and their product.  A single chunk is uploaded once.
    for (int pass = 0; pass < 2; ++pass) {
        for (size_t ch = 0; ch < n_chunks; ++ch) {
            const int64_t r0 = plan.start[ch], nr = plan.start[ch + 1] - r0, nr_pad = (nr + PAD - 1) / PAD * PAD;
            HIP_TRY(hipEventRecord(E.ev[0], st));
            if (pass == 0 || n_chunks > 1)
                if ((rc = chunk.upload(r0, nr, st))) return rc;
            HIP_TRY(hipEventRecord(E.ev[1], st));
            HIP_TRY(nabo::pca_densify_launch(chunk.d_ptr.as<int64_t>(), chunk.d_gene.as<int32_t>(), chunk.d_val.as<float>(), chunk.d_sf.as<float>(), nr,
                                             nr_pad, d_pos.as<int32_t>(), d_mu.as<double>(), d_sigma.as<double>(), d_fill.as<double>(), d_mean.as<double>(),
                                             (int)G, (int)Gp, d_y.as<double>(), st));
            HIP_TRY(hipEventRecord(E.ev[2], st));
            if (pass == 0)
                HIP_TRY(nabo::pca_colsum_launch(d_y.as<double>(), nr, (int)Gp, d_sumpart.as<double>(), d_colsum.as<double>(), st));
            else
                HIP_TRY(nabo::pca_syrk_launch(d_y.as<double>(), nr_pad, (int)Gp, d_part.as<double>(), d_acc.as<double>(), st));
            HIP_TRY(hipEventRecord(E.ev[3], st));
            HIP_TRY(hipStreamSynchronize(st));
            HIP_TRY(E.elapsed(0, 1, &ms3[0]));
            HIP_TRY(E.elapsed(1, 3, &ms3[1]));
            if (pass == 0) {
                HIP_TRY(E.elapsed(1, 3, &g_fit_phase_ms[0]));
            } else {
                HIP_TRY(E.elapsed(1, 2, &g_fit_phase_ms[1]));
                HIP_TRY(E.elapsed(2, 3, &g_fit_phase_ms[2]));
            }
        }
        if (pass == 0) {
            HIP_TRY(hipEventRecord(E.ev[0], st));
            HIP_TRY(hipMemcpyAsync(mean.data(), d_colsum.p, (size_t)G * 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipEventRecord(E.ev[1], st));
            HIP_TRY(hipStreamSynchronize(st));
            for (int64_t p = 0; p < G; ++p) {
                mean[p] = mean[p] / (double)n_rows;
                fill[p] = fill[p] - mean[p];
            }
            HIP_TRY(hipMemcpyAsync(d_mean.p, mean.data(), (size_t)G * 8, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(d_fill.p, fill.data(), (size_t)G * 8, hipMemcpyHostToDevice, st));
            HIP_TRY(hipEventRecord(E.ev[2], st));
            HIP_TRY(hipStreamSynchronize(st));
            HIP_TRY(E.elapsed(0, 1, &ms3[2]));
            HIP_TRY(E.elapsed(1, 2, &ms3[0]));
        }
    }
    HIP_TRY(hipEventRecord(E.ev[0], st));
    HIP_TRY(nabo::pca_cov_finish_launch(d_acc.as<double>(), (int)G, n_rows, d_cov.as<double>(), st));
    HIP_TRY(hipEventRecord(E.ev[1], st));
    HIP_TRY(hipMemcpyAsync(out_cov, d_cov.p, (size_t)(G * G * 8), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(E.ev[2], st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(E.elapsed(0, 1, &ms3[1]));
    HIP_TRY(E.elapsed(0, 1, &g_fit_phase_ms[2]));
    HIP_TRY(E.elapsed(1, 2, &ms3[2]));
    memcpy(out_mean, mean.data(), (size_t)G * 8);
    nabo::pca_set_device_ms(ms3, (int64_t)n_chunks);
    return NABO_OK;
}

int nabo_pca_cov_last_phase_ms(double ms[3])
{
    if (!ms) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    for (int i = 0; i < 3; ++i) ms[i] = g_fit_phase_ms[i];
    return NABO_OK;
}

}  // extern "C"
