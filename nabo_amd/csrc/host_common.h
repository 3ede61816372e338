// host_common.h -- host plumbing of the C ABI, shared by every translation unit that talks to the device: the HIP error
// check, the owning device buffer, device selection, the checks of a CSR argument, the phase timer and the creation of a
// handle.  Failures are recorded through nabo::api_fail (nabo_last_error).
#pragma once
#include <cmath>
#include <new>

#include "../../include/nabo_knn.h"
#include "launch.h"

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
