// mppi_slip.h -- the sampled-slip chain: observation-mode traversability with a draw of its own per lookup.
#pragma once
#include "mppi_geometry.h"
#include "mppi_chain.h"

namespace bn {

namespace {

// Sampled-slip helpers (BASELINE config 3, see rollout_sampled_kernel): every lookup evaluates the observation-mode
// traversability 1 - clamp(z*std + mean, 0, 1) (traversability_model.py:65-69) with its own standard normal z.
__device__ __forceinline__ float trav_from_slip(float mu, float sd, float z)
{
    const float slip = z * sd + mu;                   // Normal.sample(): normal_(0,1).mul_(std).add_(mean)
    return 1.0f - clampf(slip, 0.0f, 1.0f);
}

// Cell of a position of any magnitude, as map index (iy * G + ix) or, with the window, window index.
template <int GEO, bool LDSWIN>
__device__ __forceinline__ int slip_cell_safe(const SolveParams &p, const Win w, float x, float y)
{
    const int ix = clampi(raw_cell<GEO>(x, p.x0, p.res, p.inv_res), 0, p.G - 1);
    const int iy = clampi(raw_cell<GEO>(y, p.y0, p.res, p.inv_res), 0, p.G - 1);
    if (LDSWIN) return clampi(iy - w.wy0, 0, p.WN - 1) * p.WN + clampi(ix - w.wx0, 0, p.WN - 1);
    return iy * p.G + ix;
}

// Window cell of a position within (or a step beyond) the map limits, float domain as in trav_window.
template <int GEO>
__device__ __forceinline__ int slip_cell_window(const SolveParams &p, const Win w, float x, float y)
{
    v2f q;
    const v2f xy = {x, y}, ir = {p.inv_res, p.inv_res}, nw = {-w.fx0, -w.fy0};
    if (GEO == kGeoPow2Origin0) q = __builtin_elementwise_fma(xy, ir, nw);
    else if (GEO == kGeoPow2) q = __builtin_elementwise_fma(xy - v2f{p.x0, p.y0}, ir, nw);
    else q = quotient_general(p, xy - v2f{p.x0, p.y0}) + nw;
    const float li = clampf(floorf(q.x), 0.0f, w.fwm1);
    const float lj = clampf(floorf(q.y), 0.0f, w.fwm1);
    return (int)__builtin_fmaf(lj, w.fwn, li);
}

// One observation-mode transit (robot_model.py:59-100) of the sampled-slip chain on the LDS window of (mean, std)
// pairs: state (x, y, th) with heading (sn, cs) and window cell e advances; (xn, yn, tn) is what slot t keeps.
struct SlipChain { float x, y, th, sn, cs; int e; };

template <int GEO, bool FIRST, bool REF = false>
__device__ __forceinline__ void slip_chain_step(const SolveParams &p, const float2 *win2, const Win w, SlipChain &c, float u0,
                                                float u1, float z, float &xn, float &yn, float &tn)
{
    const float2 ms = win2[c.e];
    const float trav = trav_from_slip(ms.x, ms.y, z);                  // robot_model.py:75
    if constexpr (REF) {                                               // the reference's operation order (chain_step<..., REF>)
        float sn, cs;
        sincos_spec(c.th, sn, cs);
        const float tv = trav * u0;
        xn = c.x + (tv * cs) * p.dt;
        yn = c.y + (tv * sn) * p.dt;
        tn = c.th + (trav * u1) * p.dt;
        c.th = wrap_angle(tn);
        c.x = clampf(xn, p.x0, p.x_hi);
        c.y = clampf(yn, p.y0, p.y_hi);
        c.e = slip_cell_window<GEO>(p, w, c.x, c.y);
        return;
    }
    const float g = u0 * p.dt;                                         // the transit arithmetic of chain_step
    const float dth = trav * (u1 * p.dt);
    xn = __builtin_fmaf(trav, g * c.cs, c.x);
    yn = __builtin_fmaf(trav, g * c.sn, c.y);
    tn = theta_step(c.th, dth, FIRST);
    c.x = clampf(xn, p.x0, p.x_hi);
    c.y = clampf(yn, p.y0, p.y_hi);
    rotate_spec(c.cs, c.sn, dth);                                      // carried heading vector (bn_device_math.h)
    c.e = slip_cell_window<GEO>(p, w, c.x, c.y);
}

}  // namespace

}  // namespace bn
