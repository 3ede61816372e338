// host_common.h -- host plumbing of the C ABI, shared by every translation unit that talks to the device: the HIP error
// check, the owning device buffer, device selection, the checks of a CSR argument and of an expression matrix, the phase
// timer, the events of one call, the chunk of rows a matrix step has on the device (planned and gathered by
// row_chunks.h) and the creation of a handle.  Failures are recorded through nabo::api_fail (nabo_last_error).
#pragma once
#include <cmath>
#include <cstdio>
#include <new>
#include <vector>

#include "../../include/nabo_knn.h"
#include "launch.h"
#include "row_chunks.h"

// a failed HIP call returns NABO_E_NOMEM (out of memory) or NABO_E_HIP from the enclosing function
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e__ = (expr);                                                                   \
        if (e__ != hipSuccess) {                                                                   \
            (void)hipGetLastError(); /* (the thread's sticky copy: a later launch check must not report THIS failure) */ \
            return nabo::api_fail(e__ == hipErrorOutOfMemory ? NABO_E_NOMEM : NABO_E_HIP, "%s failed: %s", \
                                  #expr, hipGetErrorString(e__));                                  \
        }                                                                                          \
    } while (0)

namespace nabo {

// Owns one device allocation, freed by release() or with the object (`delete ix` cannot miss a member).
//   reserve: grow-only, with 1/8 + 256 B of slack; returns a NABO code (NABO_E_NOMEM on failure).
//   alloc:   exactly `bytes` (8 for none), what was held is freed first; returns the hipError_t for HIP_TRY.
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    int reserve(size_t bytes)
    {
        if (bytes <= cap) return NABO_OK;
        release();
        const size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            p = nullptr;
            return api_fail(NABO_E_NOMEM, "hipMalloc(%zu bytes) failed: %s", want, hipGetErrorString(e));
        }
        cap = want;
        return NABO_OK;
    }
    hipError_t alloc(size_t bytes)
    {
        release();
        const size_t want = bytes ? bytes : 8;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) p = nullptr;
        else cap = want;
        return e;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
};

// select `device` for the calling thread; NABO_E_NODEVICE when there is no such device
inline int use_device(int device)
{
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0)
        return api_fail(NABO_E_NODEVICE, "no HIP device is available (libnabo_knn has no CPU fallback)");
    if (device < 0 || device >= cnt) return api_fail(NABO_E_NODEVICE, "device %d out of range (have %d)", device, cnt);
    HIP_TRY(hipSetDevice(device));
    return NABO_OK;
}

// the pointer array of a compressed sparse argument: `name` [n + 1] over `major`s ("ptr" over "node"s)
inline int check_csr_ptr(const char *name, const char *major, int64_t n, const int64_t *ptr)
{
    if (!ptr) return api_fail(NABO_E_INVALID, "%s is NULL", name);
    if (ptr[0] != 0) return api_fail(NABO_E_INVALID, "%s[0] = %lld, must be 0", name, (long long)ptr[0]);
    for (int64_t i = 0; i < n; ++i)
        if (ptr[i + 1] < ptr[i]) return api_fail(NABO_E_INVALID, "%s is not monotone at %s %lld", name, major, (long long)i);
    return NABO_OK;
}

// v >= 0 and finite (-0.0 passes, a NaN does not), read off the bits: check_sparse asks it of every entry of a matrix
inline bool finite_not_negative(float v)
{
    uint32_t u;
    memcpy(&u, &v, 4);
    return u < 0x7F800000u || u == 0x80000000u;
}

// One compressed sparse matrix of expression values, `n_major` lists over `n_minor` indices ("cell" lists of "gene"s for
// rows of cells, "gene" lists of "cell"s for columns of genes): the pointers, the index range, strictly increasing
// indices within a list, and the float32 values by the step's rule -- the raw value alone (no size factors), the raw value
// and its product with the cell's size factor, or the product alone.  The size factor belongs to the cell: sf[list] for
// rows of cells (sf_by_major), sf[index] for columns of genes.  `which` ("matrix 1") is put in front of every message.
// The rule is a template argument: the loop visits every entry of the matrix on the host, and with the rule tested per
// entry the check of a projection took half as long again as with the rule compiled in.
enum SparseValues { SPARSE_RAW, SPARSE_RAW_AND_SCALED, SPARSE_SCALED };
template <SparseValues RULE>
int check_sparse(const char *which, const char *major, const char *minor, int64_t n_major, int64_t n_minor, const int64_t *ptr,
                 const int32_t *idx, const float *val, const float *sf, bool sf_by_major)
{
    char pre[32] = "", name[48];
    if (which) snprintf(pre, sizeof pre, "%s: ", which);
    snprintf(name, sizeof name, "%s%s_ptr", pre, major);
    const int rc = check_csr_ptr(name, major, n_major, ptr);
    if (rc) return rc;
    if (ptr[n_major] > 0 && (!idx || !val)) return api_fail(NABO_E_INVALID, "%s%s or val is NULL", pre, minor);
    if (RULE != SPARSE_RAW && (sf_by_major ? n_major : n_minor) > 0 && !sf) return api_fail(NABO_E_INVALID, "%ssf is NULL", pre);
    for (int64_t i = 0; i < n_major; ++i) {
        int64_t last = -1;
        for (int64_t e = ptr[i]; e < ptr[i + 1]; ++e) {
            const int64_t j = idx[e];
            if (j < 0 || j >= n_minor)
                return api_fail(NABO_E_INVALID, "%s%s[%lld] = %lld is not a %s in [0, %lld)", pre, minor, (long long)e, (long long)j, minor, (long long)n_minor);
            if (j <= last)
                return api_fail(NABO_E_INVALID, "%sthe %ss of %s %lld are not strictly increasing at entry %lld", pre, minor, major, (long long)i, (long long)e);
            last = j;
            const float v = val[e], x = RULE == SPARSE_RAW ? v : v * sf[sf_by_major ? i : j];
            if ((RULE == SPARSE_SCALED || finite_not_negative(v)) && finite_not_negative(x)) continue;
            const long long le = (long long)e, li = (long long)i, lj = (long long)j;
            if (RULE == SPARSE_RAW)
                return api_fail(NABO_E_INVALID, "%sentry %lld (%s %lld, %s %lld): value %g must be finite and >= 0", pre, le, major, li, minor, lj, (double)v);
            if (RULE == SPARSE_RAW_AND_SCALED)
                return api_fail(NABO_E_INVALID, "%sentry %lld (%s %lld, %s %lld): value %g, scaled value %g: both must be finite and >= 0", pre, le, major,
                                li, minor, lj, (double)v, (double)x);
            return api_fail(NABO_E_INVALID, "%sthe scaled value of entry %lld (%s %lld, %s %lld) is %g: values must be finite and >= 0", pre, le, major, li,
                            minor, lj, (double)x);
        }
    }
    return NABO_OK;
}

// the cells an entry point is asked for, in output order (NULL: all)
inline int check_rows(int64_t n_rows, const int64_t *rows, int64_t n_cells)
{
    for (int64_t r = 0; rows && r < n_rows; ++r)
        if (rows[r] < 0 || rows[r] >= n_cells)
            return api_fail(NABO_E_INVALID, "rows[%lld] = %lld is not a cell in [0, %lld)", (long long)r, (long long)rows[r], (long long)n_cells);
    return NABO_OK;
}

// the graph argument of a *_create entry point: ptr, nbr in [0, n) and the weights by the step's rule
enum CsrWeights { CSR_NO_WEIGHTS, CSR_FINITE, CSR_FINITE_NOT_NEGATIVE };
inline int check_csr_graph(int64_t n, const int64_t *ptr, const int64_t *nbr, const double *w, CsrWeights rule)
{
    int rc = check_csr_ptr("ptr", "node", n, ptr);
    if (rc) return rc;
    if (rule == CSR_NO_WEIGHTS) {
        if (ptr[n] > 0 && !nbr) return api_fail(NABO_E_INVALID, "nbr is NULL");
    } else if (ptr[n] > 0 && (!nbr || !w))
        return api_fail(NABO_E_INVALID, "nbr or w is NULL");
    for (int64_t e = 0; e < ptr[n]; ++e) {
        if (nbr[e] < 0 || nbr[e] >= n)
            return api_fail(NABO_E_INVALID, "nbr[%lld] = %lld is not a node in [0, %lld)", (long long)e, (long long)nbr[e], (long long)n);
        if (rule == CSR_FINITE && !std::isfinite(w[e])) return api_fail(NABO_E_INVALID, "w[%lld] is not finite", (long long)e);
        if (rule == CSR_FINITE_NOT_NEGATIVE && (!std::isfinite(w[e]) || w[e] < 0.0))
            return api_fail(NABO_E_INVALID, "w[%lld] is negative or not finite", (long long)e);
    }
    return NABO_OK;
}

// Device time of a handle's phases on the null stream: stop(which) adds the time since start() to ms[which] and to the
// total, ms[total].  ev: the handle's two events.  (Not in the host build of the sharded protocol, tests/host_shim, whose
// stand-in for HIP has no hipEventSynchronize and no use for a timer.)
#ifndef NABO_SHARDED_HOST
struct PhaseTimer {
    hipEvent_t *ev;
    double *ms;
    int total;
    int start()
    {
        HIP_TRY(hipEventRecord(ev[0], nullptr));
        return NABO_OK;
    }
    int stop(int which)
    {
        HIP_TRY(hipEventRecord(ev[1], nullptr));
        HIP_TRY(hipEventSynchronize(ev[1]));
        float t = 0;
        HIP_TRY(hipEventElapsedTime(&t, ev[0], ev[1]));
        ms[which] += t;
        ms[total] += t;
        return NABO_OK;
    }
};
#endif

// N events of one call, destroyed with the object; elapsed(a, b, into) adds the milliseconds between two recorded and
// completed events to *into.
template <int N> struct Events {
    hipEvent_t ev[N] = {};
    Events() = default;
    Events(const Events &) = delete;
    Events &operator=(const Events &) = delete;
    ~Events()
    {
        for (int i = 0; i < N; ++i)
            if (ev[i]) (void)hipEventDestroy(ev[i]);
    }
    hipError_t create()
    {
        hipError_t e = hipSuccess;
        for (int i = 0; i < N && e == hipSuccess; ++i) e = hipEventCreate(&ev[i]);
        return e;
    }
    hipError_t elapsed(int a, int b, double *into) const
    {
        float ms = 0;
        const hipError_t e = hipEventElapsedTime(&ms, ev[a], ev[b]);
        if (e == hipSuccess) *into += ms;
        return e;
    }
};

// The chunk of rows a row step (QC, projection, fit) has on the device: the caller's matrix (sf NULL: no size factors;
// rows NULL: all cells in order), the host staging of gather_rows and the device copy of the chunk's CSR.
struct RowChunk {
    const int64_t *cell_ptr;
    const int32_t *gene;
    const float *val, *sf;
    const int64_t *rows;
    std::vector<int64_t> h_ptr;
    std::vector<float> h_sf, h_val;
    std::vector<int32_t> h_gene;
    DevBuf d_ptr, d_gene, d_val, d_sf;
    // room for the largest chunk of a plan
    int reserve(int64_t max_rows, int64_t max_nnz)
    {
        HIP_TRY(d_ptr.alloc((size_t)(max_rows + 1) * 8));
        HIP_TRY(d_gene.alloc((size_t)max_nnz * 4));
        HIP_TRY(d_val.alloc((size_t)max_nnz * 4));
        if (sf) HIP_TRY(d_sf.alloc((size_t)max_rows * 4));
        h_ptr.resize((size_t)max_rows + 1);
        if (sf) h_sf.resize((size_t)max_rows);
        if (rows) {
            h_gene.resize((size_t)max_nnz);
            h_val.resize((size_t)max_nnz);
        }
        return NABO_OK;
    }
    // the rows [r0, r0 + nr) as one CSR on the device; the host staging is read until the copies have completed.
    // `gathered`, if given, is recorded between the host's gather and the copies: the start of the copies alone.
    int upload(int64_t r0, int64_t nr, hipStream_t st, hipEvent_t gathered = nullptr)
    {
        const RowSlice s = gather_rows(r0, nr, cell_ptr, gene, val, sf, rows, h_ptr.data(), h_sf.data(), h_gene.data(), h_val.data());
        if (gathered) HIP_TRY(hipEventRecord(gathered, st));
        HIP_TRY(hipMemcpyAsync(d_ptr.p, h_ptr.data(), (size_t)(nr + 1) * 8, hipMemcpyHostToDevice, st));
        if (sf) HIP_TRY(hipMemcpyAsync(d_sf.p, h_sf.data(), (size_t)nr * 4, hipMemcpyHostToDevice, st));
        if (s.nnz) {
            HIP_TRY(hipMemcpyAsync(d_gene.p, s.gene, (size_t)s.nnz * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(d_val.p, s.val, (size_t)s.nnz * 4, hipMemcpyHostToDevice, st));
        }
        return NABO_OK;
    }
};

// The tail of a *_create entry point: a new handle on `device` (selected already), filled by build(handle).  A failed host
// allocation of the build becomes NABO_E_NOMEM: nothing thrown crosses the C ABI.
template <class Handle, class Build> int create_handle(Handle **out, int device, const char *what, Build build)
{
    Handle *h = nullptr;
    int rc;
    try {
        h = new Handle;
        h->device = device;
        rc = build(h);
    } catch (const std::bad_alloc &) {
        rc = api_fail(NABO_E_NOMEM, "%s: out of host memory", what);
    }
    if (rc) {
        delete h;
        return rc;
    }
    *out = h;
    return NABO_OK;
}

}  // namespace nabo
