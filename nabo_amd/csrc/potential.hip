// Differentiation potential of the reference graph: K x = b by conjugate gradients with the Jacobi preconditioner
// (include/nabo_potential.h is the contract; nabo/_graph.py:918-954 calc_diff_potential, a dense pinv, is what it
// replaces).
//
// One iteration is five plain launches on the null stream; the scalars (rho, alpha, beta, the iteration number, the
// stop flag) live on the device and the host reads them every PT_POLL iterations:
//   product    q = K p.  A workgroup covers PT_ROWS consecutive rows; PT_GROUP lanes share a row of at most PT_LONG
//              arcs (lane l takes the arcs l, l + PT_GROUP, ..., the lanes meet in a butterfly), a longer row is left
//              to a workgroup of its own (the workgroups past the first n_blocks, one per entry of long_rows).  Each
//              workgroup adds its rows' p_i q_i into one partial sum.
//   scalar     one workgroup adds the partial sums (thread t takes t, t + PT_THREADS, ..., then a tree in LDS):
//              alpha = rho / p^T q, or the breakdown.
//   update     x += alpha p, res -= alpha q, and per workgroup the partial sums of res^T z and res^T res.
//   scalar     rho', beta, the iteration number and the stopping test.
//   direction  p = z + beta p.
// No atomics, no grid barrier: every sum has one order, so a run gives the same bits every time.  Once `done` is set
// every kernel returns at once (the direction kernel runs once more, for the iteration that set it), so iterations the
// host had queued before it read the flag change nothing.
// Components, the per-component sums of steps 2 and 5, b and the true residual's norm are taken on the host in
// ascending node id.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/nabo_potential.h"
#include "host_common.h"
#include "simple_graph.h"

namespace nabo {

constexpr int PT_THREADS = 256;
constexpr int PT_GROUP = 8;           // lanes per row of the short path
constexpr int PT_LONG = 128;          // rows of more arcs than this take a workgroup
constexpr int PT_ROWS = 256;          // rows per workgroup, and per partial sum of a dot product
constexpr int PT_POLL = 16;           // iterations queued between two reads of the scalars

enum { PT_MODE_INIT = 0, PT_MODE_ALPHA = 1, PT_MODE_BETA = 2 };

struct PotentialScalars {
    double rho, alpha, beta, pq, rr;
    long long it;
    int done, status, p_pending, pad_;
};

// the workgroup's sum of v, in every lane; s: PT_THREADS doubles, free again on return
__device__ __forceinline__ double pt_block_sum(double *s, int t, double v)
{
    s[t] = v;
    __syncthreads();
    for (int h = PT_THREADS / 2; h > 0; h >>= 1) {
        if (t < h) s[t] += s[t + h];
        __syncthreads();
    }
    const double r = s[0];
    __syncthreads();
    return r;
}

// q = K v and part[workgroup] = sum of v_i q_i over its rows; force: the product of the true residual, which runs
// whatever the stop flag says
__global__ __launch_bounds__(PT_THREADS) void pt_product_kernel(int64_t n, int64_t n_blocks, const int64_t *__restrict__ ptr,
                                                                const int32_t *__restrict__ nbr, const double *__restrict__ c,
                                                                const double *__restrict__ v, const int32_t *__restrict__ long_rows,
                                                                double *__restrict__ q, double *__restrict__ part,
                                                                const PotentialScalars *__restrict__ sc, int force)
{
    __shared__ double s[PT_THREADS];
    if (!force && sc->done) return;
    constexpr int GROUPS = PT_THREADS / PT_GROUP;
    const int t = threadIdx.x;
    double acc = 0.0;
    if ((int64_t)blockIdx.x < n_blocks) {
        const int g = t / PT_GROUP, l = t % PT_GROUP;
        const int64_t base = (int64_t)blockIdx.x * PT_ROWS;
        for (int k = 0; k < PT_ROWS / GROUPS; ++k) {
            const int64_t i = base + (int64_t)k * GROUPS + g;
            double sum = 0.0;
            bool mine = false;   // a row of this path
            if (i < n) {
                const int64_t e0 = ptr[i], e1 = ptr[i + 1];
                mine = e1 - e0 <= PT_LONG;
                if (mine)
                    for (int64_t e = e0 + l; e < e1; e += PT_GROUP) sum += v[nbr[e]];
            }
#pragma unroll
            for (int m = 1; m < PT_GROUP; m <<= 1) sum += __shfl_xor(sum, m, PT_GROUP);
            if (mine && l == 0) {
                const double vi = v[i];
                const double qi = c[i] * vi - sum;
                q[i] = qi;
                acc += vi * qi;
            }
        }
    } else {
        const int64_t i = long_rows[(int64_t)blockIdx.x - n_blocks];
        const int64_t e0 = ptr[i], e1 = ptr[i + 1];
        double sum = 0.0;
        for (int64_t e = e0 + t; e < e1; e += PT_THREADS) sum += v[nbr[e]];
        sum = pt_block_sum(s, t, sum);
        if (t == 0) {
            const double vi = v[i];
            const double qi = c[i] * vi - sum;
            q[i] = qi;
            acc = vi * qi;
        }
    }
    const double tot = pt_block_sum(s, t, acc);
    if (t == 0) part[blockIdx.x] = tot;
}

// x += alpha p, res -= alpha q; part_rz, part_rr [workgroup]: the sums of res_i z_i and res_i^2 over its rows
__global__ __launch_bounds__(PT_THREADS) void pt_update_kernel(int64_t n, const double *__restrict__ invc, const double *__restrict__ p,
                                                               const double *__restrict__ q, double *__restrict__ x, double *__restrict__ res,
                                                               double *__restrict__ part_rz, double *__restrict__ part_rr,
                                                               const PotentialScalars *__restrict__ sc)
{
    __shared__ double s[PT_THREADS];
    if (sc->done) return;
    const double alpha = sc->alpha;
    const int t = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * PT_ROWS;
    double rz = 0.0, rr = 0.0;
    for (int k = 0; k < PT_ROWS / PT_THREADS; ++k) {
        const int64_t i = base + (int64_t)k * PT_THREADS + t;
        if (i < n) {
            x[i] = x[i] + alpha * p[i];
            const double r = res[i] - alpha * q[i];
            res[i] = r;
            const double z = r * invc[i];
            rz += r * z;
            rr += r * r;
        }
    }
    rz = pt_block_sum(s, t, rz);
    rr = pt_block_sum(s, t, rr);
    if (t == 0) {
        part_rz[blockIdx.x] = rz;
        part_rr[blockIdx.x] = rr;
    }
}

// p = z + beta p, for the iteration whose second scalar step has just run
__global__ __launch_bounds__(PT_THREADS) void pt_direction_kernel(int64_t n, const double *__restrict__ invc, const double *__restrict__ res,
                                                                  double *__restrict__ p, const PotentialScalars *__restrict__ sc)
{
    if (!sc->p_pending) return;
    const double beta = sc->beta;
    const int64_t i = (int64_t)blockIdx.x * PT_THREADS + threadIdx.x;
    if (i < n) p[i] = res[i] * invc[i] + beta * p[i];
}

// one workgroup.  PT_MODE_ALPHA: a [n_a] the partial sums of p^T q.  PT_MODE_BETA, PT_MODE_INIT: a, b [n_a] those of
// res^T z and res^T res.
__global__ __launch_bounds__(PT_THREADS) void pt_scalar_kernel(int mode, int64_t n_a, const double *__restrict__ a, const double *__restrict__ b,
                                                               double tol, double bnorm, long long max_iter, PotentialScalars *sc)
{
    __shared__ double s[PT_THREADS];
    const int t = threadIdx.x;
    if (mode != PT_MODE_INIT && sc->done) {
        if (mode == PT_MODE_BETA && t == 0) sc->p_pending = 0;
        return;
    }
    double u = 0.0, w = 0.0;
    for (int64_t j = t; j < n_a; j += PT_THREADS) {
        u += a[j];
        if (mode != PT_MODE_ALPHA) w += b[j];
    }
    u = pt_block_sum(s, t, u);
    w = pt_block_sum(s, t, w);
    if (t != 0) return;
    if (mode == PT_MODE_ALPHA) {
        const double alpha = sc->rho / u;
        sc->pq = u;
        if (!(u > 0.0) || !isfinite(u) || !isfinite(alpha)) {
            sc->status = NABO_POTENTIAL_BREAKDOWN;
            sc->done = 1;
        } else
            sc->alpha = alpha;
    } else if (mode == PT_MODE_INIT) {
        sc->rho = u;
        sc->rr = w;
        sc->alpha = 0.0;
        sc->beta = 0.0;
        sc->pq = 0.0;
        sc->it = 0;
        sc->done = 0;
        sc->status = NABO_POTENTIAL_RUNNING;
        sc->p_pending = 0;
    } else {
        sc->beta = u / sc->rho;
        sc->rho = u;
        sc->rr = w;
        sc->it += 1;
        sc->p_pending = 1;
        if (sqrt(w) <= tol * bnorm) {
            sc->status = NABO_POTENTIAL_CONVERGED;
            sc->done = 1;
        } else if (sc->it >= max_iter) {
            sc->status = NABO_POTENTIAL_MAX_ITER;
            sc->done = 1;
        }
    }
}

}  // namespace nabo

using nabo::DevBuf;
using nabo::PotentialScalars;

struct nabo_potential {
    int device = 0;
    int64_t n = 0, A = 0, n_long = 0, n_blocks = 0, n_comp = 0;
    double tol = 1e-10;
    int64_t max_iter = 10000;
    std::vector<int64_t> d, c;
    std::vector<int32_t> label, comp;   // comp: the component's number, in ascending smallest member
    std::vector<int64_t> comp_size;
    std::vector<double> b;
    double bnorm = 0.0, true_rel = -1.0;
    bool prepared = false;
    PotentialScalars hs = {};
    DevBuf ptr, nbr, cd, invc, long_rows, x, res, p, q, part_a, part_b, part_c, sc;
    hipEvent_t ev[2] = {};
    double ms[4] = {0, 0, 0, 0};
    ~nabo_potential()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

namespace {

int32_t uf_find(std::vector<int32_t> &parent, int32_t i)
{
    while (parent[(size_t)i] != i) {
        parent[(size_t)i] = parent[(size_t)parent[(size_t)i]];
        i = parent[(size_t)i];
    }
    return i;
}

int potential_create(nabo_potential *H, int64_t n, const int64_t *ptr, const int64_t *nbr)
{
    // the simple graph (simple_graph.h); d counts a self-loop once, c is the row's length, the components are those of the pairs
    nabo::SimpleGraph g;
    H->n = n;
    H->d.assign((size_t)n, 0);
    std::vector<int32_t> parent((size_t)n);
    for (int64_t i = 0; i < n; ++i) parent[(size_t)i] = (int32_t)i;
    nabo::simple_graph(g, n, ptr, nbr, false, [&](size_t, int64_t a, int64_t b) {
        ++H->d[(size_t)a];
        if (a == b) return;
        ++H->d[(size_t)b];
        const int32_t ra = uf_find(parent, (int32_t)a), rb = uf_find(parent, (int32_t)b);
        if (ra != rb) parent[(size_t)std::max(ra, rb)] = std::min(ra, rb);   // the smaller root stays: a root is its component's smallest node
    });
    const std::vector<int64_t> &rptr = g.rptr;
    const std::vector<int32_t> &rnbr = g.rnbr;
    const int64_t A = rptr[(size_t)n];
    H->c.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) H->c[(size_t)i] = rptr[(size_t)i + 1] - rptr[(size_t)i];
    H->label.resize((size_t)n);
    H->comp.resize((size_t)n);
    H->comp_size.clear();
    for (int64_t i = 0; i < n; ++i) {
        const int32_t r = uf_find(parent, (int32_t)i);
        H->label[(size_t)i] = r;
        if (r == i) {   // a root comes before every other member
            H->comp[(size_t)i] = (int32_t)H->comp_size.size();
            H->comp_size.push_back(0);
        } else
            H->comp[(size_t)i] = H->comp[(size_t)r];
        ++H->comp_size[(size_t)H->comp[(size_t)i]];
    }
    H->n_comp = (int64_t)H->comp_size.size();
    const std::vector<int32_t> long_rows = nabo::long_rows(rptr, nabo::PT_LONG);
    std::vector<double> cd((size_t)n), invc((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        cd[(size_t)i] = (double)H->c[(size_t)i];
        invc[(size_t)i] = H->c[(size_t)i] ? 1.0 / (double)H->c[(size_t)i] : 0.0;
    }
    H->A = A;
    H->n_long = (int64_t)long_rows.size();
    H->n_blocks = (n + nabo::PT_ROWS - 1) / nabo::PT_ROWS;
    const size_t nb = (size_t)n * 8;
    HIP_TRY(H->ptr.alloc(nb + 8));
    HIP_TRY(H->nbr.alloc((size_t)A * 4));
    HIP_TRY(H->long_rows.alloc(long_rows.size() * 4));
    for (DevBuf *v : {&H->cd, &H->invc, &H->x, &H->res, &H->p, &H->q}) HIP_TRY(v->alloc(nb));
    HIP_TRY(H->part_a.alloc((size_t)(H->n_blocks + H->n_long) * 8));
    HIP_TRY(H->part_b.alloc((size_t)H->n_blocks * 8));
    HIP_TRY(H->part_c.alloc((size_t)H->n_blocks * 8));
    HIP_TRY(H->sc.alloc(sizeof(PotentialScalars)));
    HIP_TRY(hipMemcpy(H->ptr.p, rptr.data(), nb + 8, hipMemcpyHostToDevice));
    if (A) HIP_TRY(hipMemcpy(H->nbr.p, rnbr.data(), (size_t)A * 4, hipMemcpyHostToDevice));
    if (!long_rows.empty()) HIP_TRY(hipMemcpy(H->long_rows.p, long_rows.data(), long_rows.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(H->cd.p, cd.data(), nb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(H->invc.p, invc.data(), nb, hipMemcpyHostToDevice));
    for (hipEvent_t &e : H->ev) HIP_TRY(hipEventCreate(&e));
    return NABO_OK;
}

int product_enqueue(nabo_potential *H, const double *v, int force)
{
    hipLaunchKernelGGL(nabo::pt_product_kernel, dim3((unsigned)(H->n_blocks + H->n_long)), dim3(nabo::PT_THREADS), 0, nullptr, H->n, H->n_blocks,
                       H->ptr.as<int64_t>(), H->nbr.as<int32_t>(), H->cd.as<double>(), v, H->long_rows.as<int32_t>(), H->q.as<double>(),
                       H->part_a.as<double>(), H->sc.as<PotentialScalars>(), force);
    HIP_TRY(hipGetLastError());
    return NABO_OK;
}

int scalar_enqueue(nabo_potential *H, int mode)
{
    const bool alpha = mode == nabo::PT_MODE_ALPHA;
    hipLaunchKernelGGL(nabo::pt_scalar_kernel, dim3(1), dim3(nabo::PT_THREADS), 0, nullptr, mode, alpha ? H->n_blocks + H->n_long : H->n_blocks,
                       alpha ? H->part_a.as<double>() : H->part_b.as<double>(), H->part_c.as<double>(), H->tol, H->bnorm,
                       (long long)H->max_iter, H->sc.as<PotentialScalars>());
    HIP_TRY(hipGetLastError());
    return NABO_OK;
}

int update_enqueue(nabo_potential *H)
{
    hipLaunchKernelGGL(nabo::pt_update_kernel, dim3((unsigned)H->n_blocks), dim3(nabo::PT_THREADS), 0, nullptr, H->n, H->invc.as<double>(),
                       H->p.as<double>(), H->q.as<double>(), H->x.as<double>(), H->res.as<double>(), H->part_b.as<double>(),
                       H->part_c.as<double>(), H->sc.as<PotentialScalars>());
    HIP_TRY(hipGetLastError());
    return NABO_OK;
}

int iteration_enqueue(nabo_potential *H)
{
    int rc;
    if ((rc = product_enqueue(H, H->p.as<double>(), 0))) return rc;
    if ((rc = scalar_enqueue(H, nabo::PT_MODE_ALPHA))) return rc;
    if ((rc = update_enqueue(H))) return rc;
    if ((rc = scalar_enqueue(H, nabo::PT_MODE_BETA))) return rc;
    hipLaunchKernelGGL(nabo::pt_direction_kernel, dim3((unsigned)((H->n + nabo::PT_THREADS - 1) / nabo::PT_THREADS)), dim3(nabo::PT_THREADS), 0,
                       nullptr, H->n, H->invc.as<double>(), H->res.as<double>(), H->p.as<double>(), H->sc.as<PotentialScalars>());
    HIP_TRY(hipGetLastError());
    return NABO_OK;
}

int read_scalars(nabo_potential *H)
{
    HIP_TRY(hipMemcpy(&H->hs, H->sc.p, sizeof(PotentialScalars), hipMemcpyDeviceToHost));
    return NABO_OK;
}

int potential_prepare(nabo_potential *H, const double *r)
{
    const int64_t n = H->n;
    const size_t nb = (size_t)n * 8;
    H->prepared = false;
    H->true_rel = -1.0;
    for (double &m : H->ms) m = 0;
    // steps 2 and 3, in ascending node id
    std::vector<double> s1((size_t)H->n_comp, 0.0), ratio((size_t)H->n_comp);
    std::vector<unsigned __int128> s2((size_t)H->n_comp, 0);
    for (int64_t i = 0; i < n; ++i) {
        const double di = (double)H->d[(size_t)i];
        s1[(size_t)H->comp[(size_t)i]] += di * (r ? r[i] : 1.0);
        s2[(size_t)H->comp[(size_t)i]] += (unsigned __int128)H->d[(size_t)i] * (unsigned __int128)H->d[(size_t)i];
    }
    for (int64_t k = 0; k < H->n_comp; ++k) ratio[(size_t)k] = s1[(size_t)k] / (double)s2[(size_t)k];
    H->b.resize((size_t)n);
    std::vector<double> z((size_t)n);
    double bb = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        const double di = (double)H->d[(size_t)i];
        const double rp = (r ? r[i] : 1.0) - di * ratio[(size_t)H->comp[(size_t)i]];
        const double bi = di * rp;
        H->b[(size_t)i] = bi;
        bb += bi * bi;
        z[(size_t)i] = H->c[(size_t)i] ? bi * (1.0 / (double)H->c[(size_t)i]) : 0.0;
    }
    H->bnorm = std::sqrt(bb);
    if (!std::isfinite(H->bnorm)) return nabo::api_fail(NABO_E_INVALID, "the right-hand side overflows: ||b|| is not finite");
    nabo::PhaseTimer T{H->ev, H->ms, 3};
    int rc;
    if ((rc = T.start())) return rc;
    HIP_TRY(hipMemsetAsync(H->x.p, 0, nb, nullptr));
    HIP_TRY(hipMemsetAsync(H->q.p, 0, nb, nullptr));
    HIP_TRY(hipMemcpy(H->res.p, H->b.data(), nb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(H->p.p, z.data(), nb, hipMemcpyHostToDevice));
    PotentialScalars s0 = {};
    if (H->bnorm == 0.0) {   // x = 0 is the answer
        s0.done = 1;
        s0.status = NABO_POTENTIAL_CONVERGED;
        HIP_TRY(hipMemcpy(H->sc.p, &s0, sizeof s0, hipMemcpyHostToDevice));
    } else {
        // rho = res^T z through the kernels of an iteration: an update with alpha = 0 and q = 0 changes neither x nor res
        HIP_TRY(hipMemcpy(H->sc.p, &s0, sizeof s0, hipMemcpyHostToDevice));
        if ((rc = update_enqueue(H))) return rc;
        if ((rc = scalar_enqueue(H, nabo::PT_MODE_INIT))) return rc;
    }
    if ((rc = T.stop(0))) return rc;
    if ((rc = read_scalars(H))) return rc;
    H->prepared = true;
    return NABO_OK;
}

int potential_iterate(nabo_potential *H, int64_t count)
{
    nabo::PhaseTimer T{H->ev, H->ms, 3};
    int rc;
    if ((rc = T.start())) return rc;
    while (count > 0 && !H->hs.done) {
        const int64_t batch = std::min<int64_t>(nabo::PT_POLL, count);
        for (int64_t k = 0; k < batch; ++k)
            if ((rc = iteration_enqueue(H))) return rc;
        if ((rc = read_scalars(H))) return rc;
        count -= batch;
    }
    return T.stop(1);
}

int potential_finish(nabo_potential *H, double *V)
{
    const int64_t n = H->n;
    const size_t nb = (size_t)n * 8;
    nabo::PhaseTimer T{H->ev, H->ms, 3};
    int rc;
    if ((rc = T.start())) return rc;
    if ((rc = product_enqueue(H, H->x.as<double>(), 1))) return rc;
    std::vector<double> kx((size_t)n);
    HIP_TRY(hipMemcpy(kx.data(), H->q.p, nb, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(V, H->x.p, nb, hipMemcpyDeviceToHost));
    if ((rc = T.stop(2))) return rc;
    double tt = 0.0;
    std::vector<double> sum((size_t)H->n_comp, 0.0);
    for (int64_t i = 0; i < n; ++i) {
        const double t = H->b[(size_t)i] - kx[(size_t)i];
        tt += t * t;
        sum[(size_t)H->comp[(size_t)i]] += V[i];
    }
    H->true_rel = H->bnorm > 0.0 ? std::sqrt(tt) / H->bnorm : 0.0;
    for (int64_t k = 0; k < H->n_comp; ++k) sum[(size_t)k] = sum[(size_t)k] / (double)H->comp_size[(size_t)k];
    for (int64_t i = 0; i < n; ++i) V[i] = V[i] - sum[(size_t)H->comp[(size_t)i]];
    return NABO_OK;
}

int potential_enter(nabo_potential *H, bool need_prepared)
{
    if (!H) return nabo::api_fail(NABO_E_INVALID, "potential is NULL");
    if (need_prepared && !H->prepared) return nabo::api_fail(NABO_E_INVALID, "no prepare has finished on this handle");
    return nabo::use_device(H->device);
}

}  // namespace

extern "C" {

int nabo_potential_geometry(int32_t *group, int32_t *long_threshold, int32_t *block_rows)
{
    if (group) *group = nabo::PT_GROUP;
    if (long_threshold) *long_threshold = nabo::PT_LONG;
    if (block_rows) *block_rows = nabo::PT_ROWS;
    return NABO_OK;
}

int nabo_potential_create(nabo_potential **out, int32_t device, int64_t n, const int64_t *ptr, const int64_t *nbr)
{
    if (!out) return nabo::api_fail(NABO_E_INVALID, "out is NULL");
    *out = nullptr;
    if (n < 1) return nabo::api_fail(NABO_E_INVALID, "n=%lld must be at least 1", (long long)n);
    if (n >= ((int64_t)1 << 31)) return nabo::api_fail(NABO_E_UNSUPPORTED, "n=%lld: the potential takes fewer than 2^31 nodes", (long long)n);
    int rc = nabo::check_csr_graph(n, ptr, nbr, nullptr, nabo::CSR_NO_WEIGHTS);
    if (rc) return rc;
    // a node without an edge is an error of the input: found before any device is asked for
    {
        std::vector<uint8_t> seen((size_t)n, 0);
        for (int64_t i = 0; i < n; ++i)
            for (int64_t e = ptr[i]; e < ptr[i + 1]; ++e) seen[(size_t)i] = seen[(size_t)nbr[e]] = 1;
        for (int64_t i = 0; i < n; ++i)
            if (!seen[(size_t)i])
                return nabo::api_fail(NABO_E_INVALID, "node %lld has no edge: its row of I - A/D is a division by zero", (long long)i);
    }
    if ((rc = nabo::use_device(device))) return rc;
    return nabo::create_handle(out, device, "nabo_potential_create", [&](nabo_potential *H) { return potential_create(H, n, ptr, nbr); });
}

void nabo_potential_destroy(nabo_potential *H)
{
    if (!H) return;
    (void)hipSetDevice(H->device);
    delete H;
}

int nabo_potential_set_params(nabo_potential *H, double tol, int64_t max_iter)
{
    if (!H) return nabo::api_fail(NABO_E_INVALID, "potential is NULL");
    if (!std::isfinite(tol) || tol < 0.0) return nabo::api_fail(NABO_E_INVALID, "tol must be finite and not negative");
    if (max_iter < 1) return nabo::api_fail(NABO_E_INVALID, "max_iter=%lld must be at least 1", (long long)max_iter);
    H->tol = tol;
    H->max_iter = max_iter;
    return NABO_OK;
}

int nabo_potential_graph_size(nabo_potential *H, int64_t *n, int64_t *n_arcs, int64_t *n_long)
{
    if (!H) return nabo::api_fail(NABO_E_INVALID, "potential is NULL");
    if (n) *n = H->n;
    if (n_arcs) *n_arcs = H->A;
    if (n_long) *n_long = H->n_long;
    return NABO_OK;
}

int nabo_potential_prepare(nabo_potential *H, const double *r)
{
    if (!H) return nabo::api_fail(NABO_E_INVALID, "potential is NULL");
    if (r)
        for (int64_t i = 0; i < H->n; ++i)
            if (!std::isfinite(r[i])) return nabo::api_fail(NABO_E_INVALID, "r[%lld] is not finite", (long long)i);
    int rc = potential_enter(H, false);
    if (rc) return rc;
    return potential_prepare(H, r);
}

int nabo_potential_get_prepared(nabo_potential *H, int32_t *label, int64_t *d, int64_t *c, double *b)
{
    if (!H) return nabo::api_fail(NABO_E_INVALID, "potential is NULL");
    if (b && !H->prepared) return nabo::api_fail(NABO_E_INVALID, "no prepare has finished on this handle");
    if (label) memcpy(label, H->label.data(), (size_t)H->n * 4);
    if (d) memcpy(d, H->d.data(), (size_t)H->n * 8);
    if (c) memcpy(c, H->c.data(), (size_t)H->n * 8);
    if (b) memcpy(b, H->b.data(), (size_t)H->n * 8);
    return NABO_OK;
}

int nabo_potential_iterate(nabo_potential *H, int64_t count, int32_t *done)
{
    int rc = potential_enter(H, true);
    if (rc) return rc;
    if (count < 0) return nabo::api_fail(NABO_E_INVALID, "count=%lld is negative", (long long)count);
    rc = potential_iterate(H, count);
    if (rc) return rc;
    if (done) *done = H->hs.done;
    return NABO_OK;
}

int nabo_potential_get_state(nabo_potential *H, double *x, double *res, double *p, double *rho, int64_t *it)
{
    int rc = potential_enter(H, true);
    if (rc) return rc;
    const size_t nb = (size_t)H->n * 8;
    if (x) HIP_TRY(hipMemcpy(x, H->x.p, nb, hipMemcpyDeviceToHost));
    if (res) HIP_TRY(hipMemcpy(res, H->res.p, nb, hipMemcpyDeviceToHost));
    if (p) HIP_TRY(hipMemcpy(p, H->p.p, nb, hipMemcpyDeviceToHost));
    if ((rc = read_scalars(H))) return rc;
    if (rho) *rho = H->hs.rho;
    if (it) *it = (int64_t)H->hs.it;
    return NABO_OK;
}

int nabo_potential_set_state(nabo_potential *H, const double *x, const double *res, const double *p, double rho, int64_t it)
{
    int rc = potential_enter(H, true);
    if (rc) return rc;
    if (!x || !res || !p) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    if (!std::isfinite(rho) || it < 0) return nabo::api_fail(NABO_E_INVALID, "rho must be finite and it not negative");
    const size_t nb = (size_t)H->n * 8;
    HIP_TRY(hipMemcpy(H->x.p, x, nb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(H->res.p, res, nb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(H->p.p, p, nb, hipMemcpyHostToDevice));
    if ((rc = read_scalars(H))) return rc;
    H->hs.rho = rho;
    H->hs.it = it;
    H->hs.done = 0;
    H->hs.status = NABO_POTENTIAL_RUNNING;
    H->hs.p_pending = 0;
    HIP_TRY(hipMemcpy(H->sc.p, &H->hs, sizeof H->hs, hipMemcpyHostToDevice));
    H->true_rel = -1.0;
    return NABO_OK;
}

int nabo_potential_finish(nabo_potential *H, double *V)
{
    int rc = potential_enter(H, true);
    if (rc) return rc;
    if (!V) return nabo::api_fail(NABO_E_INVALID, "V is NULL");
    return potential_finish(H, V);
}

int nabo_potential_solve(nabo_potential *H, const double *r, double *V)
{
    if (!V) return nabo::api_fail(NABO_E_INVALID, "V is NULL");
    int rc = nabo_potential_prepare(H, r);
    if (rc) return rc;
    if ((rc = potential_iterate(H, H->max_iter))) return rc;
    return potential_finish(H, V);
}

int nabo_potential_info(nabo_potential *H, int64_t *iterations, int32_t *status, double *rel_residual, double *true_residual,
                        int64_t *n_components)
{
    if (!H) return nabo::api_fail(NABO_E_INVALID, "potential is NULL");
    if (iterations) *iterations = H->prepared ? (int64_t)H->hs.it : 0;
    if (status) *status = H->prepared ? H->hs.status : NABO_POTENTIAL_RUNNING;
    if (rel_residual) *rel_residual = H->prepared && H->bnorm > 0.0 ? std::sqrt(H->hs.rr) / H->bnorm : 0.0;
    if (true_residual) *true_residual = H->true_rel;
    if (n_components) *n_components = H->n_comp;
    return NABO_OK;
}

int nabo_potential_last_ms(nabo_potential *H, double ms[4])
{
    if (!H || !ms) return nabo::api_fail(NABO_E_INVALID, "NULL argument");
    for (int i = 0; i < 4; ++i) ms[i] = H->ms[i];
    return NABO_OK;
}

}  // extern "C"
