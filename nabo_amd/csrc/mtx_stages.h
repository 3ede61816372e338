// mtx_stages.h -- the stages the Matrix Market reader (mtx_ingest.hip) and the remap of count matrices (counts.hip)
// share on the host side: both hold (major << 32 | minor) keys with 4-byte values in two double buffers, sort them with
// mtx_sort_launch (launch.h) and get the other index by the transpose stage below.
#pragma once
#include "host_common.h"
#include "launch.h"

namespace nabo {

// sorted (major, minor) keys and their values in buffer `which` -> the (minor, major) order: ptr over the minors, the
// majors in the other key buffer's first half (the minors in its second), the values in the value buffer *which names after
inline int mtx_transpose_stage(DevBuf key[2], DevBuf val[2], int *which, int64_t nnz, int64_t n_major, int64_t n_minor, void *temp, size_t temp_bytes,
                               int64_t *d_ptr, uint32_t **d_major, hipStream_t st)
{
    uint64_t *k[2] = {key[0].as<uint64_t>(), key[1].as<uint64_t>()};
    uint32_t *v[2] = {val[0].as<uint32_t>(), val[1].as<uint32_t>()};
    HIP_TRY(mtx_sort_launch(k, v, which, nnz, n_major, n_minor, false, temp, temp_bytes, st));
    uint32_t *major = key[1 - *which].as<uint32_t>(), *minor = major + nnz;
    HIP_TRY(mtx_split_launch(k[*which], nnz, minor, major, st));
    HIP_TRY(u32_rowptr_launch(minor, nnz, n_minor, d_ptr, st));
    *d_major = major;
    return NABO_OK;
}

}  // namespace nabo
