// mppi_chain.h -- the transit chain: one UnicycleModel.transit per step, in the default and the reference-order arithmetic.
#pragma once
#include "mppi_geometry.h"

namespace bn {

namespace {

// Per-rollout recurrence state: the clamped/wrapped state t, its traversability, sin/cos of its heading.
// G, wq: what the next step can know before the traversability of its start cell arrives (chain_prepare).
struct Chain { float x, y, th, sn, cs, trav; v2f G; float wq; };

// The heading of a rollout as an OUTPUT: theta_{t+1} = wrap(theta_t + d_t) (robot_model.py:88,90), tn = the un-wrapped sum slot t
// keeps.  The first step takes the general wrap (a caller's start heading may be anything), later ones the near form.
__device__ __forceinline__ float theta_step(float &th, float dth, bool first)
{
    const float tn = th + dth;                                         // :88
    th = first ? wrap_angle(tn) : wrap_angle_near(tn);                 // :90
    return tn;
}

// One UnicycleModel.transit (robot_model.py:59-100) plus the gather for the next step.
// (xn, yn, tn) is what the reference leaves in slot t (un-clamped, un-wrapped); the chain
// advances to the clamped/wrapped state t+1.  The heading enters the positions only through (cos, sin), which are CARRIED by a
// rotation (rotate_spec); theta is integrated beside it when THETA is set (kernels whose one wave does everything).  With
// THETA = false (the role kernels' chain wave) tn returns the step's heading increment d_t instead and c.th is not touched:
// the wave that stores the trajectory integrates theta from the increments (theta_step).
// u0, u1 already lie in [u_min, u_max]: the re-clamp of robot_model.py:82-83 is the identity.
// Arithmetic of one transit (DESIGN.md "Arithmetic spec"): with g = v dt and w = omega dt (the controls, pre-scaled),
//   x~ = fma(trav, g cos, x)   y~ = fma(trav, g sin, y)   d = trav w   theta~ = theta + d
// -- the reference's ((trav v) cos) dt + x with one rounding fewer and everything but `trav` folded into factors that are ready
// before the gather returns: ONE dependent instruction between the traversability and the new position instead of four.
__device__ __forceinline__ void chain_prepare(const SolveParams &p, Chain &c, float u0, float u1)
{
    const float g = u0 * p.dt;
    c.wq = u1 * p.dt;
    c.G = v2f{g, g} * v2f{c.cs, c.sn};
}

// PREP: the caller's loop hands over the NEXT step's controls (u0n, u1n) and chain_prepare runs for them at the end of this step,
// under the gather's latency (the role kernels' chain wave); otherwise the step prepares itself from its own controls first.
// REF (BN_FLAG_REFERENCE_ORDER): the transit as the reference writes it -- sin / cos of THIS step's heading (sincos_spec), then
// x + ((trav v) cos) dt, y + ((trav v) sin) dt, theta + (trav omega) dt in that operation order (robot_model.py:86-88), the general
// heading wrap at every step (no bound on dt |omega|).  c.sn / c.cs / c.G / c.wq are not used.  The oracle's trig = 2.
template <int GEO, bool LDSWIN, bool FIRST, bool THETA = true, bool PREP = false, int ASMIDX = 0, bool REF = false>
__device__ __forceinline__ void chain_step(const SolveParams &p, const float *win, const float *__restrict__ map,
                                           const Win w, Chain &c, float u0, float u1, float &xn, float &yn, float &tn,
                                           float u0n = 0.0f, float u1n = 0.0f)
{
    if constexpr (REF) {
        static_assert(THETA && !PREP, "the reference-order step integrates its own heading");
        // (c.sn, c.cs) = sincos_spec(c.th) on entry and on exit: every caller sets them with the start heading, and the step ends with
        // the sine and cosine of the NEXT heading, issued behind the next gather.  After the first step the heading wrap takes the
        // branch-free near form where it is valid (p.wrap_near: dt max|omega| < 3; bit-identical to the general form there,
        // tests/test_gpu_device_math.py).  Same operations per value as before (round 5) -- and the same 11.7 us per
        // dependent single-instance solve: the chain wave is alone on its SIMD and issues one instruction per ~5 cycles whatever
        // they wait for, so its 46 instructions per step ARE the step (the default arithmetic has 25); the gather's latency was
        // already covered.  The price of this arithmetic on the latency path stays 1.36x; `value_reference_order` reports it.
        const float tv = c.trav * u0;
        xn = c.x + (tv * c.cs) * p.dt;                                 // :86
        yn = c.y + (tv * c.sn) * p.dt;                                 // :87
        tn = c.th + (c.trav * u1) * p.dt;                              // :88
        c.x = clampf(xn, p.x0, ASMIDX >= 2 ? w.xhi_v : p.x_hi);        // :93
        c.y = clampf(yn, p.y0, ASMIDX >= 2 ? w.yhi_v : p.y_hi);        // :94
        c.trav = LDSWIN ? trav_window<GEO, ASMIDX>(p, win, w, c.x, c.y) : trav_lookup<GEO, false, false>(p, win, map, w, c.x, c.y);
        __builtin_amdgcn_sched_barrier(0);
        c.th = (!FIRST && p.wrap_near) ? wrap_angle_near(tn) : wrap_angle(tn);      // :90
        sincos_spec(c.th, c.sn, c.cs);
        return;
    }
    if (!PREP) chain_prepare(p, c, u0, u1);
    // Position strand first: update, clamp, cell index, and the gather goes out; the heading strand (rotation, 7
    // instructions) then runs under the gather's LDS latency.  The scheduling barrier keeps the compiler from
    // interleaving the two again (it used to issue the gather two thirds into the step).
    const float dth = c.trav * c.wq;                                   // :88
    const v2f pos = __builtin_elementwise_fma(v2f{c.trav, c.trav}, c.G, v2f{c.x, c.y});   // :86-87, x and y in lockstep
    xn = pos.x;
    yn = pos.y;
    c.x = clampf(xn, p.x0, ASMIDX >= 2 ? w.xhi_v : p.x_hi);            // :93   (ASMIDX 2, 3: the upper limits in vector registers the caller keeps)
    c.y = clampf(yn, p.y0, ASMIDX >= 2 ? w.yhi_v : p.y_hi);            // :94
    c.trav = LDSWIN ? trav_window<GEO, ASMIDX>(p, win, w, c.x, c.y) : trav_lookup<GEO, false, false>(p, win, map, w, c.x, c.y);
    __builtin_amdgcn_sched_barrier(0);
    if (THETA) tn = theta_step(c.th, dth, FIRST); else tn = dth;
    rotate_spec<ASMIDX == 2>(c.cs, c.sn, dth, w.c0_v);
    if (PREP) chain_prepare(p, c, u0n, u1n);
}

}  // namespace

}  // namespace bn
