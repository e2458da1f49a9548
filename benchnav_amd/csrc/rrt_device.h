// rrt_device.h -- device code the RRT kernels (rrt_kernels.hip) and the closed-loop RRT kernels (clrrt_kernels.hip) share: the
// norm of Tree.nearest_neighbor / _is_goal_reached, the 64-bit (value bits, index) minimum, the sample kernel (the instance's
// MT19937 stream parsed into the sample of every iteration) and the near-goal pick of the path kernels.  Internal linkage, like
// mt19937.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bn_device_math.h"
#include "mt19937.h"

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

constexpr int kTreeSampleThreads = 256;    // >= 227 (mt19937.h)

struct TreeSampleArgs {
    const uint64_t *seeds;     // (B), read when reseed
    uint32_t *state;           // (B, 624) the block of the stream being read
    int32_t *pos;              // (B) the next word in it, 624 = twist first
    const float *goals;        // (B, DIM)
    float *samples;            // (B, iters, DIM)
    int32_t *flags;            // (B, iters) 1 where the sample is the goal
    int iters, reseed;
    float rate, xspan, x0, yspan, y0;      // f32(rate), f32(x1 - x0), f32(x0), f32(y1 - y0), f32(y0)
    const int32_t *active;     // (B) or nullptr = every instance: an instance whose word is 0 returns before touching anything
};

// torch's MT19937 stream of the instance (seeded, or reloaded from the handle), parsed into the sample of every iteration: one
// uniform u; u < f32(rate) -> the goal, else DIM more uniforms -> (x, y) and for DIM == 3 the heading f32(f32(u 2) pi).  Neither
// planner's steer feeds back into the draws, so the sample sequence does not depend on the tree.  The state goes back to the handle.
template <int DIM>
__global__ __launch_bounds__(kTreeSampleThreads) void tree_samples_kernel(TreeSampleArgs a)
{
    static_assert(DIM == 2 || DIM == 3, "positions are (x, y) or (x, y, heading)");
    __shared__ uint32_t mt[2][kMtN];
    const int b = blockIdx.x, t = threadIdx.x;
    if (a.active && a.active[b] == 0) return;              // (uniform over the workgroup: no barrier is left waiting)
    int pos = kMtN;
    if (a.reseed) {
        if (t == 0) mt_seed(mt[0], (uint32_t)a.seeds[b]);
    } else {
        for (int i = t; i < kMtN; i += kTreeSampleThreads) mt[0][i] = a.state[(size_t)b * kMtN + i];
        pos = min(max(a.pos[b], 0), kMtN);
    }
    __syncthreads();
    MtStream s{mt, 0, pos};
    const float gx = a.goals[DIM * b], gy = a.goals[DIM * b + 1], gth = DIM == 3 ? a.goals[DIM * b + 2] : 0.0f;
    float *out = a.samples + (size_t)b * a.iters * DIM;
    int32_t *fl = a.flags + (size_t)b * a.iters;
    // every thread walks the same words (the parse is a dependent chain: 1 or 1 + DIM draws per iteration); they take turns to write
    for (int it = 0; it < a.iters; ++it) {
        const bool goal = mt_next(s) < a.rate;
        float x = gx, y = gy, th = gth;
        if (!goal) {
            x = __fadd_rn(__fmul_rn(mt_next(s), a.xspan), a.x0);
            y = __fadd_rn(__fmul_rn(mt_next(s), a.yspan), a.y0);
            if (DIM == 3) th = __fmul_rn(__fmul_rn(mt_next(s), 2.0f), kPi);
        }
        if (t == (it & (kTreeSampleThreads - 1))) {
            out[DIM * it] = x;
            out[DIM * it + 1] = y;
            if (DIM == 3) out[DIM * it + 2] = th;
            fl[it] = goal ? 1 : 0;
        }
    }
    for (int i = t; i < kMtN; i += kTreeSampleThreads) a.state[(size_t)b * kMtN + i] = s.mt[s.cur][i];
    if (t == 0) a.pos[b] = s.pos;
}

struct NearGoal {
    int total;                 // nodes within the threshold
    unsigned long long key;    // (cost bits << 32) | index of the pick among them, ~0 where there is none
};

// _is_goal_reached over the n nodes (rows of STRIDE floats that start with x, y), by a workgroup of THREADS: the nodes with
// norm(node - goal) < f32(threshold), and among them the lowest cost, then the lowest index (costs are >= +0: their bit
// patterns order as unsigned integers).  Every thread gets the same result; the barrier inside orders the kernel's LDS use.
template <int STRIDE, int THREADS>
__device__ __forceinline__ NearGoal near_goal_pick(const float *nodes, const float *costs, int n, float gx, float gy, float threshold)
{
    __shared__ unsigned long long part[THREADS / 64];
    __shared__ int cnt[THREADS / 64];
    unsigned long long key = ~0ull;
    int near = 0;
    for (int i = threadIdx.x; i < n; i += THREADS) {
        float px, py;
        if (STRIDE == 2) {
            const float2 p = ((const float2 *)nodes)[i];
            px = p.x; py = p.y;
        } else {
            px = nodes[STRIDE * i]; py = nodes[STRIDE * i + 1];
        }
        if (rrt_norm(__fsub_rn(px, gx), __fsub_rn(py, gy)) < threshold) {
            ++near;
            const unsigned long long k = ((unsigned long long)__float_as_uint(costs[i]) << 32) | (unsigned)i;
            key = k < key ? k : key;
        }
    }
    for (int m = 32; m > 0; m >>= 1) near += __shfl_xor(near, m, 64);
    if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6] = near;
    key = block_min_u64<THREADS>(key, part);                                           // its barrier covers cnt[] too
    int total = 0;
    for (int w = 0; w < THREADS / 64; ++w) total += cnt[w];
    return NearGoal{total, key};
}

}  // namespace
}  // namespace bn
