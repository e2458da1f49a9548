// torch's CPU generator on the device: MT19937 seeded with the low 32 bits of the seed, one float32
// uniform f32(r & 0xFFFFFF) 2^-24 per 32-bit output r.  Shared by the terrain generator's draws (terrain_kernels.hip) and the RRT
// planner's samples (rrt_kernels.hip).  The 624-word state lives in LDS twice (the block being read and the block being built);
// every thread of the workgroup follows the same control flow on the same LDS words, so the barriers stay uniform.  The
// workgroup needs at least 227 threads: each of the twist's parallel segments is one word per thread.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace bn {
namespace {

constexpr int kMtN = 624, kMtM = 397;

// init_genrand(seed): a dependent chain, made by one thread
__device__ __forceinline__ void mt_seed(uint32_t *mt, uint32_t x)
{
    mt[0] = x;
    for (int i = 1; i < kMtN; ++i) {
        x = 1812433253u * (x ^ (x >> 30)) + (uint32_t)i;
        mt[i] = x;
    }
}

__device__ __forceinline__ uint32_t mt_mix(uint32_t hi, uint32_t lo)
{
    const uint32_t y = (hi & 0x80000000u) | (lo & 0x7fffffffu);
    return (y >> 1) ^ ((y & 1u) ? 0x9908B0DFu : 0u);
}

__device__ __forceinline__ float mt_uniform(uint32_t y)
{
    y ^= y >> 11;
    y ^= (y << 7) & 0x9D2C5680u;
    y ^= (y << 15) & 0xEFC60000u;
    y ^= y >> 18;
    return __fmul_rn((float)(y & 0xFFFFFFu), 5.9604644775390625e-08f);       // exact: 24 bits times 2^-24
}

struct MtStream {
    uint32_t (*mt)[kMtN];      // LDS, two blocks
    int cur, pos;              // the block being read and the next word in it: the same in every thread
};

// The next 624 words from mt[cur] into mt[cur ^ 1], in the twist's four dependent segments.  Every thread of the block calls it.
// mt[cur ^ 1] was last read before the previous refill's barriers, so nobody still reads what this one writes.
__device__ void mt_refill(MtStream &s)
{
    const uint32_t *o = s.mt[s.cur];
    uint32_t *n = s.mt[s.cur ^ 1];
    const int t = threadIdx.x;
    if (t < kMtN - kMtM) n[t] = o[t + kMtM] ^ mt_mix(o[t], o[t + 1]);                                    // i < 227
    __syncthreads();
    if (t < kMtN - kMtM) n[t + 227] = n[t] ^ mt_mix(o[t + 227], o[t + 228]);                             // 227 <= i < 454
    __syncthreads();
    if (t < 169) n[t + 454] = n[t + 227] ^ mt_mix(o[t + 454], o[t + 455]);                               // 454 <= i < 623
    __syncthreads();
    if (t == 0) n[623] = n[396] ^ mt_mix(o[623], n[0]);
    __syncthreads();
    s.cur ^= 1;
    s.pos = 0;
}

__device__ __forceinline__ uint32_t mt_word(MtStream &s)
{
    if (s.pos == kMtN) mt_refill(s);
    return s.mt[s.cur][s.pos++];
}

__device__ __forceinline__ float mt_next(MtStream &s) { return mt_uniform(mt_word(s)); }

}  // namespace
}  // namespace bn
