// umap_common.h -- what the UMAP fit (umap.hip) and the UMAP transform (umap_transform.hip) share of their definitions
// (include/nabo_umap.h): the hash's mix and its constant G, the sum by a binary tree over a lane group, and the clip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nabo {

constexpr uint64_t UM_GOLD = 0x9E3779B97F4A7C15ull;

__host__ __device__ __forceinline__ uint64_t umap_mix(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// TREE over the W lanes of a group (W a power of two): adjacent lanes first; every lane ends with the same bits
template <int W> __device__ __forceinline__ double umap_tree(double v)
{
#pragma unroll
    for (int m = 1; m < W; m <<= 1) v += __shfl_xor(v, m, W);
    return v;
}

__device__ __forceinline__ double umap_clip(double v) { return v > 4.0 ? 4.0 : v < -4.0 ? -4.0 : v; }

}  // namespace nabo
