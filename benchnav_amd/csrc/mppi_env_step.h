// mppi_env_step.h -- one PlanetaryEnv.step on the device: what follows a solve in an episode (MPPI, A* + DWA, CL-RRT loops).
#pragma once
#include "mppi_geometry.h"

namespace bn {

namespace {

// One PlanetaryEnv.step (planetary_env.py:189-219) for instance b: observation-mode transit with the
// latent slip sampled at the current cell (traversability_model.py:65-69: Normal(mean, std)[cell].sample()
// = z * std + mean), then the goal test.  Like the reference, a terminated environment keeps moving when stepped again;
// with p.env_freeze (opt-in, for fixed-length batched episodes) an instance already within goal_thr of its goal stays put.
// Every workgroup that needs the next state evaluates this itself: same inputs, same operations.
struct EnvStep { float x, y, th, reward; bool reached, frozen; };

// The latent slip model at the cell of (sx, sy): the two loads of env_advance, issued on their own so that a caller who knows the
// state early can have them in flight while it waits for the control.
struct EnvCell { float mean, std; };

template <int GEO>
__device__ __forceinline__ EnvCell env_fetch(const SolveParams &p, int b, float sx, float sy)
{
    const int ix = clampi(raw_cell<GEO>(sx, p.x0, p.res, p.inv_res), 0, p.G - 1);
    const int iy = clampi(raw_cell<GEO>(sy, p.y0, p.res, p.inv_res), 0, p.G - 1);
    const size_t cell = (size_t)b * p.map_stride + (size_t)iy * p.G + ix;
    return EnvCell{p.lat_mean[cell], p.lat_std[cell]};
}

template <int GEO>
__device__ __forceinline__ EnvStep env_advance_with(const SolveParams &p, int b, float sx, float sy, float sth, float u0, float u1,
                                                    const float *z_ptr, uint64_t step, const EnvCell lc)
{
    const float gx = p.goal[b * 2 + 0], gy = p.goal[b * 2 + 1];
    EnvStep r;
    const float d0x = sx - gx, d0y = sy - gy;
    r.frozen = p.env_freeze && sqrt_cr(d0x * d0x + d0y * d0y) < p.goal_thr;      // terminated at an earlier step
    float z;
    if (z_ptr) {
        z = z_ptr[b];
    } else {
        const u32x4 q = philox4x32_10(u32x4{(uint32_t)b, (uint32_t)step, (uint32_t)(step >> 32), 0x454e5631u},
                                      (uint32_t)p.env_seed, (uint32_t)(p.env_seed >> 32));
        float z1;
        box_muller(q.x, q.y, z, z1);
    }
    const float slip = z * lc.std + lc.mean;
    const float trav = 1.0f - clampf(slip, 0.0f, 1.0f);
    const float v = clampf(u0, p.umin0, p.umax0), om = clampf(u1, p.umin1, p.umax1);   // robot_model.py:82-83
    float sn, cs;
    sincos_spec(sth, sn, cs);
    const float xn = sx + ((trav * v) * cs) * p.env_dt;
    const float yn = sy + ((trav * v) * sn) * p.env_dt;
    const float tn = sth + (trav * om) * p.env_dt;
    r.x = r.frozen ? sx : clampf(xn, p.x0, p.x_hi);
    r.y = r.frozen ? sy : clampf(yn, p.y0, p.y_hi);
    r.th = r.frozen ? sth : wrap_angle(tn);
    r.reward = trav;
    const float dx = r.x - gx, dy = r.y - gy;
    r.reached = sqrt_cr(dx * dx + dy * dy) < p.goal_thr;             // planetary_env.py:215-217
    return r;
}

template <int GEO>
__device__ __forceinline__ EnvStep env_advance(const SolveParams &p, int b, float sx, float sy, float sth, float u0, float u1,
                                               const float *z_ptr, uint64_t step)
{
    return env_advance_with<GEO>(p, b, sx, sy, sth, u0, u1, z_ptr, step, env_fetch<GEO>(p, b, sx, sy));
}

}  // namespace

}  // namespace bn
