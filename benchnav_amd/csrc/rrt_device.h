// rrt_device.h -- device functions the RRT kernels (rrt_kernels.hip) and the closed-loop RRT kernels (clrrt_kernels.hip) share: the
// norm of Tree.nearest_neighbor / _is_goal_reached and the 64-bit (value bits, index) minimum.  Internal linkage, like mt19937.h.
#pragma once
#include <hip/hip_runtime.h>

namespace bn {
namespace {

__device__ __forceinline__ float rrt_norm(float dx, float dy)
{
    return sqrtf(__builtin_fmaf(dy, dy, __fmul_rn(dx, dx)));
}

template <int THREADS>
__device__ __forceinline__ unsigned long long block_min_u64(unsigned long long key, unsigned long long *part)
{
    for (int m = 32; m > 0; m >>= 1) {
        const unsigned long long o = __shfl_xor(key, m, 64);
        key = o < key ? o : key;
    }
    if (THREADS > 64) {
        // part[] is written here and read before the barrier that ends the caller's iteration: the next write comes after that barrier
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = key;
        __syncthreads();
        key = part[0];
        for (int w = 1; w < THREADS / 64; ++w) key = part[w] < key ? part[w] : key;
    }
    return key;
}

}  // namespace
}  // namespace bn
