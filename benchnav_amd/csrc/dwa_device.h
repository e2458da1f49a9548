// dwa_device.h -- the DWA step's device code (reference src/planners/local_planners/dwa.py:116-285), shared by the stand-alone
// kernels of DWA.forward (mppi_kernels.hip: dwa_window_kernel, dwa_kernel) and the fused A* + DWA episode (astar_dwa.hip).  One
// definition of every operation, so the two paths agree bit for bit by construction.  Internal linkage like the MPPI kernels'
// headers, of which it takes the lookups (mppi_geometry.h), the transit step (mppi_chain.h) and the wave reductions (mppi_sync.h).
#pragma once
#include "mppi_geometry.h"
#include "mppi_chain.h"
#include "mppi_sync.h"

namespace bn {

namespace {

// ------------------------------------------------------------------------------
// Dynamic window (dwa.py:168-199): lo = max(u_min, prev - a_lim * dt), hi = min(u_max, prev + a_lim * dt) around the previous
// first control; vs = linspace(lo_v, hi_v, nv), ws = linspace(lo_w, hi_w, nw); actions = cartesian_prod(vs, ws) (v major).
// linspace as ATen's scalar kernel computes it: step = (end - start) / (n - 1); element i < n/2 is start + step * i, the others
// end - step * (n - 1 - i).  (On AVX2 hosts torch's vectorised path evaluates the first 8 elements from `start` alone, so torch
// itself is machine dependent in the last bit; this is the form AVX-512 hosts and every scalar tail use.)
// ------------------------------------------------------------------------------
__device__ __forceinline__ float linspace_at(float start, float end, int n, int i)
{
    if (n == 1) return start;
    const float step = (end - start) / (float)(n - 1);
    return i < n / 2 ? start + step * (float)i : end - step * (float)(n - 1 - i);
}

struct DwaWindow { float lo0, hi0, lo1, hi1; };

__device__ __forceinline__ DwaWindow dwa_window(const SolveParams &p, float pv, float pw, float alim0, float alim1, float dwa_dt)
{
    return DwaWindow{fmaxf(p.umin0, pv - alim0 * dwa_dt), fminf(p.umax0, pv + alim0 * dwa_dt),
                     fmaxf(p.umin1, pw - alim1 * dwa_dt), fminf(p.umax1, pw + alim1 * dwa_dt)};
}

// the (nv * nw, 2) candidate grid of one instance into act
__device__ __forceinline__ void dwa_window_actions(const DwaWindow &d, int nv, int nw, float *act, int tid, int nthreads)
{
    for (int k = tid; k < nv * nw; k += nthreads) {
        const int iv = k / nw, iw = k - iv * nw;
        act[2 * k + 0] = linspace_at(d.lo0, d.hi0, nv, iv);
        act[2 * k + 1] = linspace_at(d.lo1, d.hi1, nw, iw);
    }
}

// ------------------------------------------------------------------------------
// Sub-goal (dwa.py:240-244 + 260-285), evaluated like the reference on candidate 0's ALIASED slot-0 state: _compute_costs calls
// _select_sub_goal(state_seq_batch[0, 0, :]) after the rollouts, and transit's in-place update (robot_model.py:86-88) has by then
// made it the start state advanced by one un-clamped, un-wrapped step of candidate 0 = (lo_v, lo_w).  The pick: the nearest path
// point with |bearing| < pi/2 and distance > lookahead -- the FIRST point over all points at that distance -- else the path's end.
// ------------------------------------------------------------------------------
template <int GEO>
__device__ __forceinline__ void dwa_subgoal_state(const SolveParams &p, int b, float sx, float sy, float sth, const DwaWindow &d, int nv,
                                                  int nw, float &x, float &y, float &th)
{
    const float *__restrict__ map = p.map + (size_t)b * p.map_stride;
    const Win w{0, 0, 0.f, 0.f, 0.f, 0.f};
    const float trav = trav_lookup<GEO, false, true>(p, nullptr, map, w, sx, sy);
    const float v = clampf(linspace_at(d.lo0, d.hi0, nv, 0), p.umin0, p.umax0), om = clampf(linspace_at(d.lo1, d.hi1, nw, 0), p.umin1, p.umax1);
    float sn, cs;
    sincos_spec(sth, sn, cs);
    x = sx + ((trav * v) * cs) * p.dt;
    y = sy + ((trav * v) * sn) * p.dt;
    th = sth + (trav * om) * p.dt;
}

// distance of the path point (px, py) from (x, y) (dwa.py:270-271)
__device__ __forceinline__ float dwa_point_dist(float px, float py, float x, float y)
{
    const float dx = px - x, dy = py - y;
    return sqrt_cr(dx * dx + dy * dy);
}

// the bearing's atan2 (dwa.py:272): one definition, so that the test hook (bn_device_math_eval fn 6) evaluates the very function
__device__ __forceinline__ float dwa_bearing_atan2(float dy, float dx)
{
    return atan2f(dy, dx);
}

// ... and whether it is a candidate: ahead (|bearing| < 90 deg) and beyond the look-ahead distance (dwa.py:272-277); INFINITY if not
__device__ __forceinline__ float dwa_ahead_dist(float px, float py, float x, float y, float th, float lookahead)
{
    const float dx = px - x, dy = py - y;
    const float dist = sqrt_cr(dx * dx + dy * dy);
    const float ang = dwa_bearing_atan2(dy, dx) - th;
    return (fabsf(ang) < kPi / 2.0f && dist > lookahead) ? dist : INFINITY;
}

// Minimum over the workgroup (nthreads a multiple of 64, at most 1024); red holds nthreads / 64 floats.  Ends with every lane
// holding the result; red may be reused after the next barrier.
__device__ __forceinline__ float block_min(float v, float *red, int tid, int nthreads)
{
    v = -wave_max(-v);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    float m = red[0];
    for (int i = 1; i < (nthreads >> 6); ++i) m = fminf(m, red[i]);
    return m;
}

__device__ __forceinline__ int block_min_i(int v, int *redi, int tid, int nthreads)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    if ((tid & 63) == 0) redi[tid >> 6] = v;
    __syncthreads();
    int m = redi[0];
    for (int i = 1; i < (nthreads >> 6); ++i) m = min(m, redi[i]);
    return m;
}

// ------------------------------------------------------------------------------
// Candidate rollouts, costs, argmin and weights of one instance (dwa.py:116-153, 224-258).  NA constant-control candidates act
// (NA, 2) are rolled out with the same transit / aliasing as MPPI (dwa.py:224-227), costed with the stage cost against the sub-goal
// (hx, hy) and the terminal cost against the goal (gx, gy), accumulated in fp32 in step order like `cost_batch +=` (dwa.py:251-256);
// argmin = first minimum (dwa.py:139), weights = softmax(-cost) (dwa.py:151).  Lane = candidate; the workgroup has nthreads >= NA
// lanes (a multiple of 64).  win: the LDS window (LDSWIN), red: 16 floats then 16 ints of LDS.  Xb / cost_b / w_b (this instance's
// rows) may be null.  Returns the argmin, the same in every lane.  The caller's next write of win or red must follow a barrier.
// ------------------------------------------------------------------------------
template <int GEO, bool LDSWIN>
__device__ __forceinline__ int dwa_rollout_argmin(const SolveParams &p, int b, float sx, float sy, float sth, const float *act, int NA,
                                                  float hx, float hy, float gx, float gy, float *win, float *red, int tid, int nthreads,
                                                  float *Xb, float *cost_b, float *w_b)
{
    const int T = p.T;
    int *redi = reinterpret_cast<int *>(red + 16);
    const float *__restrict__ map = p.map + (size_t)b * p.map_stride;
    Win w{0, 0, 0.f, 0.f, 0.f, 0.f};
    if (LDSWIN) {
        w = window_origin<GEO>(p, sx, sy);
        stage_window(win, map, w, p.WN, p.G, tid, nthreads);
    }
    __syncthreads();
    const bool active = tid < NA;
    const int k = active ? tid : NA - 1;
    const float u0 = clampf(act[k * 2 + 0], p.umin0, p.umax0);       // transit re-clamps (robot_model.py:82-83)
    const float u1 = clampf(act[k * 2 + 1], p.umin1, p.umax1);
    Chain c;
    c.x = sx; c.y = sy; c.th = sth;
    sincos_spec(c.th, c.sn, c.cs);
    c.trav = trav_lookup<GEO, LDSWIN, true>(p, win, map, w, c.x, c.y);
    float *Xk = Xb ? Xb + (size_t)k * (T + 1) * 3 : nullptr;
    float cost = 0.0f;
    const bool ref = p.ref_order != 0;
    for (int t = 0; t < T; ++t) {
        float xn, yn, tn;
        if (ref && t == 0) chain_step<GEO, LDSWIN, true, true, false, 0, true>(p, win, map, w, c, u0, u1, xn, yn, tn);
        else if (ref) chain_step<GEO, LDSWIN, false, true, false, 0, true>(p, win, map, w, c, u0, u1, xn, yn, tn);
        else if (t == 0) chain_step<GEO, LDSWIN, true>(p, win, map, w, c, u0, u1, xn, yn, tn);
        else chain_step<GEO, LDSWIN, false>(p, win, map, w, c, u0, u1, xn, yn, tn);
        if (Xk && active) { Xk[3 * t] = xn; Xk[3 * t + 1] = yn; Xk[3 * t + 2] = tn; }
        const float dx = xn - hx, dy = yn - hy;
        cost = cost + (sqrt_cr(dx * dx + dy * dy) + (c.trav <= p.thr ? 1.0e4f : 0.0f));      // objectives.py:47-53
    }
    if (Xk && active) { Xk[3 * T] = c.x; Xk[3 * T + 1] = c.y; Xk[3 * T + 2] = c.th; }
    const float dxT = c.x - gx, dyT = c.y - gy;
    cost = cost + (sqrt_cr(dxT * dxT + dyT * dyT) + (c.trav <= p.thr ? 1.0e4f : 0.0f));       // dwa.py:256
    if (cost_b && active) cost_b[tid] = cost;

    // argmin with first-index tie break, then softmax(-cost)
    float cm = active ? cost : INFINITY;
    int im = active ? tid : 0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float oc = __shfl_xor(cm, o);
        const int oi = __shfl_xor(im, o);
        if (oc < cm || (oc == cm && oi < im)) { cm = oc; im = oi; }
    }
    const int wv = tid >> 6, nw = nthreads >> 6;
    if ((tid & 63) == 0) { red[wv] = cm; redi[wv] = im; }
    __syncthreads();
    float cmin = red[0];
    int imin = redi[0];
    for (int i = 1; i < nw; ++i)
        if (red[i] < cmin || (red[i] == cmin && redi[i] < imin)) { cmin = red[i]; imin = redi[i]; }
    if (w_b) {
        __syncthreads();
        const float e = active ? expf((-cost) - (-cmin)) : 0.0f;
        float es = wave_sum(e);
        if ((tid & 63) == 0) red[wv] = es;
        __syncthreads();
        float tot = 0.0f;
        for (int i = 0; i < nw; ++i) tot += red[i];
        if (active) w_b[tid] = e / tot;
    }
    return imin;
}

}  // namespace

}  // namespace bn
