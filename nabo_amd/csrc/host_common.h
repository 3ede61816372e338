// host_common.h -- host plumbing of the C ABI, shared by every translation unit that talks to the device: the HIP error
// check, the owning device buffer and device selection.  Failures are recorded through nabo::api_fail (nabo_last_error).
#pragma once
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

}  // namespace nabo
