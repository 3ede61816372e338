// ForceAtlas2 layout of the reference graph with the repulsion summed over every pair (include/nabo_layout.h is the
// contract; nabo/_graph.py:179-237 set_ref_layout is what it replaces).
//
// One iteration is five kernels on one stream, with no host round trip: pack (float64 state -> float32 x, y, mass),
// repulsion (the all-pairs sum: the hot path), node (gravity, attraction, the force, swinging and traction with
// per-block partial sums), speed (the final tree and the global speed: one thread) and move.
//
// Repulsion.  A workgroup of 256 lanes owns LAY_IBLOCK = 1024 nodes i, four per lane, and walks a split of the j tiles.
// A tile of LAY_JTILE = 256 nodes (x, y, mass, 0: 16 B each) is staged in LDS and read by broadcast: every lane reads
// the same address, one ds_read_b128 serves the lane's four pairs.  Per pair: two subtractions, a multiply, an fma, the
// clamp (one v_max_f32: it makes j = i, coincident nodes and the padding contribute exactly 0 without a branch), v_rcp_f32,
// a multiply by mass_j and two fmas; scaling_ratio * mass_i is applied once per node in the node kernel.  Sums are float32
// within a tile and float64 across tiles.  The packed array is padded to a multiple of LAY_IBLOCK with mass 0 at
// (0, 0), so neither the i loads nor the tile loads need a bound.  No atomics: every (split, node) has one writer.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/nabo_layout.h"
#include "host_common.h"
#include "simple_graph.h"

namespace nabo {

constexpr int LAY_THREADS = 256;
constexpr int LAY_IPL = 4;                            // nodes i per lane
constexpr int LAY_IBLOCK = LAY_THREADS * LAY_IPL;     // nodes i per workgroup
constexpr int LAY_JTILE = 256;                        // nodes j per staged tile: one per lane
constexpr int LAY_WG_TARGET = 2048;                   // workgroups wanted of the repulsion grid (8 per CU)
constexpr int LAY_MAX_SPLITS = 64;

// the tiles of n nodes and how they are split over blockIdx.y: a function of n alone
static void layout_splits(int64_t n, int *ntiles, int *tiles_per_split, int *nsplit)
{
    const int64_t nib = (n + LAY_IBLOCK - 1) / LAY_IBLOCK;
    const int nt = (int)((n + LAY_JTILE - 1) / LAY_JTILE);
    int64_t want = (LAY_WG_TARGET + nib - 1) / nib;
    want = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(want, LAY_MAX_SPLITS), nt));
    const int tps = (int)((nt + want - 1) / want);
    *ntiles = nt;
    *tiles_per_split = tps;
    *nsplit = (nt + tps - 1) / tps;
}

__global__ __launch_bounds__(LAY_THREADS) void layout_pack_kernel(const double *__restrict__ x, const double *__restrict__ y,
                                                                  const double *__restrict__ mass, int64_t n, int64_t npad,
                                                                  float4 *__restrict__ pk)
{
    const int64_t i = (int64_t)blockIdx.x * LAY_THREADS + threadIdx.x;
    if (i >= npad) return;
    float4 p = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (i < n) p = make_float4((float)x[i], (float)y[i], (float)mass[i], 0.0f);
    pk[i] = p;
}

__global__ __launch_bounds__(LAY_THREADS) void layout_repulse_kernel(const float4 *__restrict__ pk, int64_t n, int ntiles,
                                                                     int tiles_per_split, double *__restrict__ part,
                                                                     const LayoutScalars *__restrict__ sc)
{
    if (sc->stop) return;
    __shared__ float4 tile[LAY_JTILE];
    const int t = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * LAY_IBLOCK + t;
    float xi[LAY_IPL], yi[LAY_IPL];
    double ax[LAY_IPL], ay[LAY_IPL];
#pragma unroll
    for (int k = 0; k < LAY_IPL; ++k) {
        const float4 p = pk[i0 + k * LAY_THREADS];
        xi[k] = p.x;
        yi[k] = p.y;
        ax[k] = ay[k] = 0.0;
    }
    const int tile0 = blockIdx.y * tiles_per_split;
    const int tile1 = min(ntiles, tile0 + tiles_per_split);
    float4 nxt = pk[(int64_t)tile0 * LAY_JTILE + t];
    for (int tl = tile0; tl < tile1; ++tl) {
        __syncthreads();   // the readers of the previous tile are done
        tile[t] = nxt;
        __syncthreads();
        if (tl + 1 < tile1) nxt = pk[(int64_t)(tl + 1) * LAY_JTILE + t];
        float sx[LAY_IPL], sy[LAY_IPL];
#pragma unroll
        for (int k = 0; k < LAY_IPL; ++k) sx[k] = sy[k] = 0.0f;
#pragma unroll 8
        for (int jj = 0; jj < LAY_JTILE; ++jj) {
            const float4 q = tile[jj];
#pragma unroll
            for (int k = 0; k < LAY_IPL; ++k) {
                const float ddx = xi[k] - q.x, ddy = yi[k] - q.y;
                const float d2 = __builtin_fmaxf(__builtin_fmaf(ddy, ddy, ddx * ddx), 0x1p-100f);
                const float f = q.z * __builtin_amdgcn_rcpf(d2);
                sx[k] = __builtin_fmaf(ddx, f, sx[k]);
                sy[k] = __builtin_fmaf(ddy, f, sy[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < LAY_IPL; ++k) {
            ax[k] += (double)sx[k];
            ay[k] += (double)sy[k];
        }
    }
    double *px = part + (int64_t)blockIdx.y * 2 * n, *py = px + n;
#pragma unroll
    for (int k = 0; k < LAY_IPL; ++k) {
        const int64_t i = i0 + k * LAY_THREADS;
        if (i < n) {
            px[i] = ax[k];
            py[i] = ay[k];
        }
    }
}

// S and T by the same tree: sS[0], sT[0] hold the block's sums on return (all 256 lanes call it)
__device__ __forceinline__ void layout_tree(double *sS, double *sT, int t, double s, double tr)
{
    sS[t] = s;
    sT[t] = tr;
    __syncthreads();
    for (int h = LAY_THREADS / 2; h > 0; h >>= 1) {
        if (t < h) {
            sS[t] += sS[t + h];
            sT[t] += sT[t + h];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(LAY_THREADS) void layout_node_kernel(int64_t n, const double *__restrict__ x, const double *__restrict__ y,
                                                                  const double *__restrict__ mass, double *__restrict__ dx,
                                                                  double *__restrict__ dy, const int64_t *__restrict__ ptr,
                                                                  const int32_t *__restrict__ nbr, const double *__restrict__ ew,
                                                                  const double *__restrict__ part, int nsplit, LayoutParams P,
                                                                  double *__restrict__ f_rep, double *__restrict__ f_grav,
                                                                  double *__restrict__ f_attr, double *__restrict__ swing,
                                                                  double *__restrict__ block_st, const LayoutScalars *__restrict__ sc)
{
    if (sc->stop) return;
    __shared__ double sS[LAY_THREADS], sT[LAY_THREADS];
    const int t = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * LAY_THREADS + t;
    double sw = 0.0, tr = 0.0;
    if (i < n) {
        const double xi = x[i], yi = y[i], mi = mass[i];
        double rx = 0.0, ry = 0.0;
        for (int s = 0; s < nsplit; ++s) {
            rx += part[(int64_t)s * 2 * n + i];
            ry += part[(int64_t)s * 2 * n + n + i];
        }
        const double c = P.scaling_ratio * mi;
        rx = c * rx;
        ry = c * ry;
        const double r = sqrt(xi * xi + yi * yi);
        double gf = 0.0;
        if (r > 0.0) gf = P.strong ? P.scaling_ratio * mi * P.gravity : mi * P.gravity / r;
        const double gx = -(xi * gf), gy = -(yi * gf);
        double axx = 0.0, ayy = 0.0;
        for (int64_t e = ptr[i]; e < ptr[i + 1]; ++e) {
            const int64_t j = nbr[e];
            double f = -P.comp * ew[e];
            if (P.oad) f /= mass[j < i ? j : i];
            axx += (xi - x[j]) * f;
            ayy += (yi - y[j]) * f;
        }
        const double ox = dx[i], oy = dy[i];
        const double nx = (rx + gx) + axx, ny = (ry + gy) + ayy;
        dx[i] = nx;
        dy[i] = ny;
        f_rep[2 * i] = rx;
        f_rep[2 * i + 1] = ry;
        f_grav[2 * i] = gx;
        f_grav[2 * i + 1] = gy;
        f_attr[2 * i] = axx;
        f_attr[2 * i + 1] = ayy;
        const double a = ox - nx, b = oy - ny, p = ox + nx, q = oy + ny;
        sw = mi * sqrt(a * a + b * b);
        tr = 0.5 * mi * sqrt(p * p + q * q);
        swing[i] = sw;
    }
    layout_tree(sS, sT, t, sw, tr);
    if (t == 0) {
        block_st[2 * (int64_t)blockIdx.x] = sS[0];
        block_st[2 * (int64_t)blockIdx.x + 1] = sT[0];
    }
}

__global__ __launch_bounds__(LAY_THREADS) void layout_speed_kernel(int64_t n, const double *__restrict__ block_st, int64_t nblocks,
                                                                   double jitter_tolerance, LayoutScalars *__restrict__ sc)
{
    if (sc->stop) return;
    __shared__ double sS[LAY_THREADS], sT[LAY_THREADS];
    const int t = threadIdx.x;
    double s = 0.0, tr = 0.0;
    for (int64_t b = t; b < nblocks; b += LAY_THREADS) {
        s += block_st[2 * b];
        tr += block_st[2 * b + 1];
    }
    layout_tree(sS, sT, t, s, tr);
    if (t != 0) return;
    const double S = sS[0], T = sT[0];
    sc->S = S;
    sc->T = T;
    if (S == 0.0 || T == 0.0) {
        sc->stop = 1;
        return;
    }
    double speed = sc->speed, eff = sc->eff;
    const double nn = (double)n;
    const double est = 0.05 * sqrt(nn);
    double jt = jitter_tolerance * fmax(sqrt(est), fmin(10.0, est * T / (nn * nn)));
    if (S / T > 2.0) {
        if (eff > 0.05) eff *= 0.5;
        jt = fmax(jt, jitter_tolerance);
    }
    const double target = jt * eff * T / S;
    if (S > jt * T) {
        if (eff > 0.05) eff *= 0.7;
    } else if (speed < 1000.0)
        eff *= 1.3;
    speed += fmin(target - speed, 0.5 * speed);
    sc->speed = speed;
    sc->eff = eff;
}

__global__ __launch_bounds__(LAY_THREADS) void layout_move_kernel(int64_t n, double *__restrict__ x, double *__restrict__ y,
                                                                  const double *__restrict__ dx, const double *__restrict__ dy,
                                                                  const double *__restrict__ swing, LayoutScalars *__restrict__ sc)
{
    if (sc->stop) return;
    const int64_t i = (int64_t)blockIdx.x * LAY_THREADS + threadIdx.x;
    if (i < n) {
        const double speed = sc->speed;
        const double f = speed / (1.0 + sqrt(speed * swing[i]));
        x[i] += dx[i] * f;
        y[i] += dy[i] * f;
    }
    if (i == 0) sc->done += 1;
}

int layout_iblock() { return LAY_IBLOCK; }
int layout_jtile() { return LAY_JTILE; }

hipError_t layout_pack_launch(const double *x, const double *y, const double *mass, int64_t n, int64_t npad, void *pk, hipStream_t st)
{
    hipLaunchKernelGGL(layout_pack_kernel, dim3((unsigned)(npad / LAY_THREADS)), dim3(LAY_THREADS), 0, st, x, y, mass, n, npad,
                       reinterpret_cast<float4 *>(pk));
    return hipGetLastError();
}

hipError_t layout_repulse_launch(const void *pk, int64_t n, double *part, const LayoutScalars *sc, hipStream_t st)
{
    int ntiles, tps, nsplit;
    layout_splits(n, &ntiles, &tps, &nsplit);
    const unsigned nib = (unsigned)((n + LAY_IBLOCK - 1) / LAY_IBLOCK);
    hipLaunchKernelGGL(layout_repulse_kernel, dim3(nib, (unsigned)nsplit), dim3(LAY_THREADS), 0, st,
                       reinterpret_cast<const float4 *>(pk), n, ntiles, tps, part, sc);
    return hipGetLastError();
}

hipError_t layout_node_launch(int64_t n, const double *x, const double *y, const double *mass, double *dx, double *dy,
                              const int64_t *ptr, const int32_t *nbr, const double *ew, const double *part, const LayoutParams &P,
                              double *f_rep, double *f_grav, double *f_attr, double *swing, double *block_st,
                              const LayoutScalars *sc, hipStream_t st)
{
    int ntiles, tps, nsplit;
    layout_splits(n, &ntiles, &tps, &nsplit);
    hipLaunchKernelGGL(layout_node_kernel, dim3((unsigned)((n + LAY_THREADS - 1) / LAY_THREADS)), dim3(LAY_THREADS), 0, st, n, x, y,
                       mass, dx, dy, ptr, nbr, ew, part, nsplit, P, f_rep, f_grav, f_attr, swing, block_st, sc);
    return hipGetLastError();
}

hipError_t layout_speed_launch(int64_t n, const double *block_st, double jitter_tolerance, LayoutScalars *sc, hipStream_t st)
{
    hipLaunchKernelGGL(layout_speed_kernel, dim3(1), dim3(LAY_THREADS), 0, st, n, block_st, (n + LAY_THREADS - 1) / LAY_THREADS,
                       jitter_tolerance, sc);
    return hipGetLastError();
}

hipError_t layout_move_launch(int64_t n, double *x, double *y, const double *dx, const double *dy, const double *swing,
                              LayoutScalars *sc, hipStream_t st)
{
    hipLaunchKernelGGL(layout_move_kernel, dim3((unsigned)((n + LAY_THREADS - 1) / LAY_THREADS)), dim3(LAY_THREADS), 0, st, n, x, y,
                       dx, dy, swing, sc);
    return hipGetLastError();
}

}  // namespace nabo

using nabo::DevBuf;

namespace {
constexpr int LAY_TIMED = 16;   // iterations of a run that are timed kernel by kernel (its last ones)
}

struct nabo_layout {
    int device = 0;
    int64_t n = 0, npad = 0, n_arcs = 0;
    int nsplit = 1;
    std::vector<double> h_w;   // the simple graph's weights in row order, what ew is made from
    bool ew_stale = true, ran = false;
    int oad = 1, strong = 0;
    double ewi = 1.0, jitter = 1.0, scaling = 1.0, gravity = 1.0, mean_mass = 1.0;
    DevBuf x, y, dx, dy, mass, pk, part, ptr, nbr, ew, f_rep, f_grav, f_attr, swing, block_st, sc;
    hipEvent_t ev[LAY_TIMED * 6 + 2] = {};
    double ms[6] = {0, 0, 0, 0, 0, 0};
    int64_t n_timed = 0;
    ~nabo_layout()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

namespace {

int layout_upload_scalars(nabo_layout *L, double speed, double eff)
{
    nabo::LayoutScalars h;
    memset(&h, 0, sizeof h);
    h.speed = speed;
    h.eff = eff;
    HIP_TRY(hipMemcpy(L->sc.p, &h, sizeof h, hipMemcpyHostToDevice));
    return NABO_OK;
}

int layout_create(nabo_layout *L, int64_t n, const int64_t *ptr, const int64_t *nbr, const double *w)
{
    // the simple graph (simple_graph.h); a node's mass is 1 + its pairs, a self-loop counting once
    nabo::SimpleGraph g;
    std::vector<double> mass((size_t)n, 1.0);
    nabo::simple_graph(g, n, ptr, nbr, true, [&](size_t, int64_t a, int64_t b) {
        mass[(size_t)a] += 1.0;
        if (a != b) mass[(size_t)b] += 1.0;
    });
    double msum = 0.0;
    for (int64_t i = 0; i < n; ++i) msum += mass[(size_t)i];
    L->mean_mass = msum / (double)n;
    const std::vector<int64_t> &rptr = g.rptr;
    const std::vector<int32_t> &rnbr = g.rnbr;
    const int64_t A = rptr[(size_t)n];
    L->h_w.resize((size_t)A);
    for (size_t s = 0; s < (size_t)A; ++s) L->h_w[s] = w[g.last[(size_t)g.slot_pair[s]]];
    L->n = n;
    L->n_arcs = A;
    L->npad = (n + nabo::LAY_IBLOCK - 1) / nabo::LAY_IBLOCK * nabo::LAY_IBLOCK;
    int ntiles, tps;
    nabo::layout_splits(n, &ntiles, &tps, &L->nsplit);
    const size_t nb = (size_t)n * 8;
    for (DevBuf *b : {&L->x, &L->y, &L->dx, &L->dy, &L->mass, &L->swing}) HIP_TRY(b->alloc(nb));
    for (DevBuf *b : {&L->f_rep, &L->f_grav, &L->f_attr}) HIP_TRY(b->alloc(2 * nb));
    HIP_TRY(L->pk.alloc((size_t)L->npad * 16));
    HIP_TRY(L->part.alloc((size_t)L->nsplit * 2 * nb));
    HIP_TRY(L->ptr.alloc(((size_t)n + 1) * 8));
    HIP_TRY(L->nbr.alloc((size_t)A * 4));
    HIP_TRY(L->ew.alloc((size_t)A * 8));
    HIP_TRY(L->block_st.alloc((size_t)((n + nabo::LAY_THREADS - 1) / nabo::LAY_THREADS) * 16));
    HIP_TRY(L->sc.alloc(sizeof(nabo::LayoutScalars)));
    for (DevBuf *b : {&L->x, &L->y, &L->dx, &L->dy}) HIP_TRY(hipMemset(b->p, 0, nb));
    HIP_TRY(hipMemcpy(L->mass.p, mass.data(), nb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(L->ptr.p, rptr.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice));
    if (A) HIP_TRY(hipMemcpy(L->nbr.p, rnbr.data(), (size_t)A * 4, hipMemcpyHostToDevice));
    for (hipEvent_t &e : L->ev) HIP_TRY(hipEventCreate(&e));
    return layout_upload_scalars(L, 1.0, 1.0);
}

}  // namespace

extern "C" {

int nabo_layout_geometry(int64_t n, int32_t *i_block, int32_t *j_tile, int32_t *n_splits)
{
    if (n < 1) return nabo::api_fail(NABO_E_INVALID, "n=%lld must be at least 1", (long long)n);
    int ntiles, tps, nsplit;
    nabo::layout_splits(n, &ntiles, &tps, &nsplit);
    if (i_block) *i_block = nabo::LAY_IBLOCK;
    if (j_tile) *j_tile = nabo::LAY_JTILE;
    if (n_splits) *n_splits = nsplit;
    return NABO_OK;
}

int nabo_layout_create(nabo_layout **out, int32_t device, int64_t n, const int64_t *ptr, const int64_t *nbr, const double *w)
{
    if (!out) return nabo::api_fail(NABO_E_INVALID, "out is NULL");
    *out = nullptr;
    if (n < 1) return nabo::api_fail(NABO_E_INVALID, "n=%lld must be at least 1", (long long)n);
    if (n >= ((int64_t)1 << 24)) return nabo::api_fail(NABO_E_UNSUPPORTED, "n=%lld: the layout takes fewer than 2^24 nodes", (long long)n);
    int rc = nabo::check_csr_graph(n, ptr, nbr, w, nabo::CSR_FINITE);
    if (rc) return rc;
    if ((rc = nabo::use_device(device))) return rc;
    return nabo::create_handle(out, device, "nabo_layout_create", [&](nabo_layout *L) { return layout_create(L, n, ptr, nbr, w); });
}

void nabo_layout_destroy(nabo_layout *L)
{
    if (!L) return;
    (void)hipSetDevice(L->device);
    delete L;
}

int nabo_layout_set_params(nabo_layout *L, int32_t outbound_attraction_distribution, double edge_weight_influence,
                           double jitter_tolerance, double scaling_ratio, int32_t strong_gravity_mode, double gravity,
                           double barnes_hut_theta)
{
    if (!L) return nabo::api_fail(NABO_E_INVALID, "layout is NULL");
    (void)barnes_hut_theta;
    if (!std::isfinite(edge_weight_influence) || !std::isfinite(jitter_tolerance) || !std::isfinite(scaling_ratio) || !std::isfinite(gravity))
        return nabo::api_fail(NABO_E_INVALID, "a layout parameter is not finite");
    L->ew_stale = L->ew_stale || edge_weight_influence != L->ewi;
    L->oad = outbound_attraction_distribution != 0;
    L->strong = strong_gravity_mode != 0;
    L->ewi = edge_weight_influence;
    L->jitter = jitter_tolerance;
    L->scaling = scaling_ratio;
    L->gravity = gravity;
    return NABO_OK;
}

int nabo_layout_set_state(nabo_layout *L, const double *x, const double *y, const double *dx, const double *dy, double speed,
                          double eff)
{
    if (!L) return nabo::api_fail(NABO_E_INVALID, "layout is NULL");
    if (!x || !y || (!dx) != (!dy)) return nabo::api_fail(NABO_E_INVALID, "x or y is NULL, or only one of dx, dy is given");
    if (!std::isfinite(speed) || !std::isfinite(eff)) return nabo::api_fail(NABO_E_INVALID, "speed or eff is not finite");
    int rc = nabo::use_device(L->device);
    if (rc) return rc;
    const size_t nb = (size_t)L->n * 8;
    HIP_TRY(hipMemcpy(L->x.p, x, nb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(L->y.p, y, nb, hipMemcpyHostToDevice));
    if (dx) {
        HIP_TRY(hipMemcpy(L->dx.p, dx, nb, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(L->dy.p, dy, nb, hipMemcpyHostToDevice));
    } else {
        HIP_TRY(hipMemset(L->dx.p, 0, nb));
        HIP_TRY(hipMemset(L->dy.p, 0, nb));
    }
    return layout_upload_scalars(L, speed, eff);
}

int nabo_layout_get_state(nabo_layout *L, double *x, double *y, double *dx, double *dy, double *speed, double *eff)
{
    if (!L) return nabo::api_fail(NABO_E_INVALID, "layout is NULL");
    int rc = nabo::use_device(L->device);
    if (rc) return rc;
    const size_t nb = (size_t)L->n * 8;
    if (x) HIP_TRY(hipMemcpy(x, L->x.p, nb, hipMemcpyDeviceToHost));
    if (y) HIP_TRY(hipMemcpy(y, L->y.p, nb, hipMemcpyDeviceToHost));
    if (dx) HIP_TRY(hipMemcpy(dx, L->dx.p, nb, hipMemcpyDeviceToHost));
    if (dy) HIP_TRY(hipMemcpy(dy, L->dy.p, nb, hipMemcpyDeviceToHost));
    nabo::LayoutScalars h;
    HIP_TRY(hipMemcpy(&h, L->sc.p, sizeof h, hipMemcpyDeviceToHost));
    if (speed) *speed = h.speed;
    if (eff) *eff = h.eff;
    return NABO_OK;
}

int nabo_layout_run(nabo_layout *L, int64_t n_iter, int64_t *done)
{
    if (!L) return nabo::api_fail(NABO_E_INVALID, "layout is NULL");
    if (n_iter < 0) return nabo::api_fail(NABO_E_INVALID, "n_iter=%lld is negative", (long long)n_iter);
    if (done) *done = 0;
    int rc = nabo::use_device(L->device);
    if (rc) return rc;
    for (double &m : L->ms) m = 0;
    L->n_timed = 0;
    if (n_iter == 0) return NABO_OK;
    if (L->ew_stale) {
        std::vector<double> e(L->h_w.size());
        for (size_t i = 0; i < e.size(); ++i) e[i] = L->ewi == 0.0 ? 1.0 : L->ewi == 1.0 ? L->h_w[i] : pow(L->h_w[i], L->ewi);
        if (!e.empty()) HIP_TRY(hipMemcpy(L->ew.p, e.data(), e.size() * 8, hipMemcpyHostToDevice));
        L->ew_stale = false;
    }
    nabo::LayoutScalars h;
    HIP_TRY(hipMemcpy(&h, L->sc.p, sizeof h, hipMemcpyDeviceToHost));
    rc = layout_upload_scalars(L, h.speed, h.eff);   // done = 0, stop = 0
    if (rc) return rc;
    nabo::LayoutParams P;
    P.scaling_ratio = L->scaling;
    P.gravity = L->gravity;
    P.comp = L->oad ? L->mean_mass : 1.0;
    P.oad = L->oad;
    P.strong = L->strong;
    hipStream_t st = nullptr;
    nabo::LayoutScalars *sc = L->sc.as<nabo::LayoutScalars>();
    const int64_t n = L->n, first_timed = n_iter > LAY_TIMED ? n_iter - LAY_TIMED : 0;
    hipEvent_t *run_ev = L->ev + LAY_TIMED * 6;
    HIP_TRY(hipEventRecord(run_ev[0], st));
    for (int64_t it = 0; it < n_iter; ++it) {
        hipEvent_t *ev = it >= first_timed ? L->ev + (it - first_timed) * 6 : nullptr;
        if (ev) HIP_TRY(hipEventRecord(ev[0], st));
        HIP_TRY(nabo::layout_pack_launch(L->x.as<double>(), L->y.as<double>(), L->mass.as<double>(), n, L->npad, L->pk.p, st));
        if (ev) HIP_TRY(hipEventRecord(ev[1], st));
        HIP_TRY(nabo::layout_repulse_launch(L->pk.p, n, L->part.as<double>(), sc, st));
        if (ev) HIP_TRY(hipEventRecord(ev[2], st));
        HIP_TRY(nabo::layout_node_launch(n, L->x.as<double>(), L->y.as<double>(), L->mass.as<double>(), L->dx.as<double>(),
                                         L->dy.as<double>(), L->ptr.as<int64_t>(), L->nbr.as<int32_t>(), L->ew.as<double>(),
                                         L->part.as<double>(), P, L->f_rep.as<double>(), L->f_grav.as<double>(),
                                         L->f_attr.as<double>(), L->swing.as<double>(), L->block_st.as<double>(), sc, st));
        if (ev) HIP_TRY(hipEventRecord(ev[3], st));
        HIP_TRY(nabo::layout_speed_launch(n, L->block_st.as<double>(), L->jitter, sc, st));
        if (ev) HIP_TRY(hipEventRecord(ev[4], st));
        HIP_TRY(nabo::layout_move_launch(n, L->x.as<double>(), L->y.as<double>(), L->dx.as<double>(), L->dy.as<double>(),
                                         L->swing.as<double>(), sc, st));
        if (ev) HIP_TRY(hipEventRecord(ev[5], st));
    }
    HIP_TRY(hipEventRecord(run_ev[1], st));
    HIP_TRY(hipStreamSynchronize(st));
    L->ran = true;
    HIP_TRY(hipMemcpy(&h, L->sc.p, sizeof h, hipMemcpyDeviceToHost));
    if (done) *done = h.done;
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, run_ev[0], run_ev[1]));
    L->ms[5] = ms;
    L->n_timed = n_iter - first_timed;
    for (int64_t k = 0; k < L->n_timed; ++k)
        for (int j = 0; j < 5; ++j) {
            HIP_TRY(hipEventElapsedTime(&ms, L->ev[k * 6 + j], L->ev[k * 6 + j + 1]));
            L->ms[j] += ms / (double)L->n_timed;
        }
    return NABO_OK;
}

int nabo_layout_last_forces(nabo_layout *L, double *repulsion, double *gravity, double *attraction, double st[2])
{
    if (!L) return nabo::api_fail(NABO_E_INVALID, "layout is NULL");
    if (!L->ran) return nabo::api_fail(NABO_E_INVALID, "no iteration has run on this layout");
    int rc = nabo::use_device(L->device);
    if (rc) return rc;
    const size_t nb = (size_t)L->n * 16;
    if (repulsion) HIP_TRY(hipMemcpy(repulsion, L->f_rep.p, nb, hipMemcpyDeviceToHost));
    if (gravity) HIP_TRY(hipMemcpy(gravity, L->f_grav.p, nb, hipMemcpyDeviceToHost));
    if (attraction) HIP_TRY(hipMemcpy(attraction, L->f_attr.p, nb, hipMemcpyDeviceToHost));
    if (st) {
        nabo::LayoutScalars h;
        HIP_TRY(hipMemcpy(&h, L->sc.p, sizeof h, hipMemcpyDeviceToHost));
        st[0] = h.S;
        st[1] = h.T;
    }
    return NABO_OK;
}

int nabo_layout_last_ms(nabo_layout *L, double ms[6], int64_t *n_timed)
{
    if (!L || !ms) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    for (int i = 0; i < 6; ++i) ms[i] = L->ms[i];
    if (n_timed) *n_timed = L->n_timed;
    return NABO_OK;
}

}  // extern "C"
