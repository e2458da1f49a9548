// mppi_noise.h -- the noise of a rollout (the library's Philox stream or the caller's arrays) and the perturbed controls made of it.
#pragma once
#include "mppi_kernels.h"
#include "bn_device_math.h"

namespace bn {

namespace {

// Producer: the clamped perturbed controls of steps t and t+1 (t even) of this lane's rollout,
//   u = clamp(mean + sigma * eps, u_min, u_max)          mppi.py:152-157
// written to the LDS control tile (and to HBM when _perturbed_action_seqs is materialised).
template <int EPS, bool STORE_U>
__device__ __forceinline__ void produce_pair(const SolveParams &p, const float *__restrict__ eps, int b, int kk, int t,
                                             uint64_t solve, const float *ml, float *Ul, float *Ub, size_t Kp, int lane)
{
    float e[4];
    const int t1 = min(t + 1, p.T - 1);
    if (EPS == kEpsPhilox) {
        philox_eps_pair(p.seed, solve, (uint32_t)b, (uint32_t)(kk + p.k0), (uint32_t)(t >> 1), e);
    } else if (EPS == kEpsKT2) {
        const float *row = eps + ((size_t)b * p.K + kk) * p.T * 2;
        const float2 v0 = *reinterpret_cast<const float2 *>(row + 2 * t);
        const float2 v1 = *reinterpret_cast<const float2 *>(row + 2 * t1);
        e[0] = v0.x; e[1] = v0.y; e[2] = v1.x; e[3] = v1.y;
    } else {
        const float *r0 = eps + ((size_t)b * p.T + t) * 2 * p.K;
        const float *r1 = eps + ((size_t)b * p.T + t1) * 2 * p.K;
        e[0] = r0[kk]; e[1] = r0[p.K + kk]; e[2] = r1[kk]; e[3] = r1[p.K + kk];
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int tt = t + s;
        if (tt < p.T) {
            const float u0 = clampf(ml[2 * tt] + p.sigma0 * e[2 * s], p.umin0, p.umax0);
            const float u1 = clampf(ml[2 * tt + 1] + p.sigma1 * e[2 * s + 1], p.umin1, p.umax1);
            Ul[(2 * tt) * kUPad + lane] = u0;
            Ul[(2 * tt + 1) * kUPad + lane] = u1;
            if (STORE_U) { float *Ut = Ub + (size_t)(2 * tt) * Kp; Ut[0] = u0; Ut[Kp] = u1; }
        }
    }
}


// The noise of steps t and t+1 (t even) of rollout kk: the library's Philox stream or the caller's arrays.  (The same three-way fetch as
// in produce_pair, for p.eps and p.solve.  Written twice: one function for both changed the one-wave kernel's code, profiles/mppi_device_split.txt.)
template <int EPS, bool FRESH_KEYS = false>
__device__ __forceinline__ void noise_pair(const SolveParams &p, int b, int kk, int t, float e[4])
{
    const int t1 = min(t + 1, p.T - 1);
    if (EPS == kEpsPhilox) {
        philox_eps_pair<FRESH_KEYS>(p.seed, p.solve, (uint32_t)b, (uint32_t)(kk + p.k0), (uint32_t)(t >> 1), e);
    } else if (EPS == kEpsKT2) {
        const float *row = p.eps + ((size_t)b * p.K + kk) * p.T * 2;
        const float2 v0 = *reinterpret_cast<const float2 *>(row + 2 * t);
        const float2 v1 = *reinterpret_cast<const float2 *>(row + 2 * t1);
        e[0] = v0.x; e[1] = v0.y; e[2] = v1.x; e[3] = v1.y;
    } else {
        const float *r0 = p.eps + ((size_t)b * p.T + t) * 2 * p.K;
        const float *r1 = p.eps + ((size_t)b * p.T + t1) * 2 * p.K;
        e[0] = r0[kk]; e[1] = r0[p.K + kk]; e[2] = r1[kk]; e[3] = r1[p.K + kk];
    }
}

}  // namespace

}  // namespace bn
