// The closed-loop RRT planner for B instances per launch: `CLRRT` of the reference (src/planners/global_planners/sampling_based/
// cl_rrt.py, with Dubins and PurePursuit of src/planners/local_planners) on the device.  One workgroup of ONE wave
// per instance: everything a closed-loop step does is at most 64 wide (a truncated reference path has at most 64 points).
//   tree_samples_kernel<3> (rrt_device.h) the sample of every iteration: one uniform u; u < f32(rate) -> the goal node (x, y,
//                          heading), else three more uniforms -> (x, y, theta).  An infeasible steer only `continue`s, so the
//                          sequence does not depend on the tree.
//   clrrt_grow_kernel      per iteration: nearest node on (x, y) (rrt_device.h), the steer, and where it is feasible the append.
//                          x, y, heading, cost and the two integrals of every node live in LDS; sequences go straight to global.
//   clrrt_steer_kernel     one steer per instance from a given state, controller state and target, with no tree: the teacher-forced
//                          comparison with the reference, with the truncated path and the target index of every step written out.
//   clrrt_path_kernel      goal test and pick (near_goal_pick, rrt_device.h: lowest cost, then lowest index), parent walk,
//                          concatenation of the segments.
// One steer (clrrt_steer): the six Dubins words in float32 as NumPy evaluates them on float32 scalars (each transcendental is the
// float64 function rounded to float32), lane p = path point p in float64 from its arc length 0.25 p, a sequential float64 sum of the
// segment lengths for the truncation, then the serial follow loop: validity mask on the lanes, first set lane, PID in float64, the
// float32 cast of the action, the library's reference-order transit (chain_step<..., REF>) and costs in float32.
// Every loop is bounded (iterations, max_seqs, 64 points, the parent walk by the node count); no workgroup waits for another.
// The map: one for all instances (bn_clrrt_set_map: SolveParams.map_stride 0) or one per instance (bn_clrrt_set_instance_maps:
// stride G * G over a buffer of B maps); clrrt_steer is the only reader, instance b at p.map + b * p.map_stride.
// The host side is written with bn_host.h (guard, HIP check, buffer table) and shares its plan steps with RRT (rrt_host.h).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/benchnav_mppi.h"
#include "clrrt_view.h"
#include "dwa_device.h"
#include "rrt_host.h"

namespace bn {
namespace {

constexpr int kClrrtThreads = 64;          // the growth and steer kernels: one wave
constexpr int kClrrtPathThreads = 256;
constexpr int kClrrtPoints = 64;           // path points a steer can hold: bn_clrrt_create bounds delta_distance accordingly
constexpr int kClrrtResult = 6;            // found, picked node, path length, near-goal count, error, node count
static_assert(kClrrtResult == kClrrtResultWords, "clrrt_view.h: the follow kernel reads the result rows");
constexpr int kClrrtSteerResult = 4;       // feasible, length, word, points
constexpr int kClrrtMaxNodes = 2048;       // 24 bytes of LDS per node
constexpr float kHalfPi32 = 1.57079637050628662f;      // f32(pi / 2)
constexpr double kPi64 = 3.141592653589793, kTwoPi64 = 6.283185307179586;

// NumPy's float32 functions on float32 scalars, taken as the float64 function rounded once more (correctly rounded but for
// double rounding); NumPy's own are within an ulp of that (DESIGN.md 4.7 has what the difference costs).
__device__ __forceinline__ void sincos32(float a, float &s, float &c)
{
    double sd, cd;
    sincos((double)a, &sd, &cd);
    s = (float)sd; c = (float)cd;
}
__device__ __forceinline__ float atan2_32(float y, float x) { return (float)atan2((double)y, (double)x); }
// a % f32(2 pi) with the sign of the divisor (np.remainder): fmod is exact, the fix-up addition rounds in float32
__device__ __forceinline__ float mod2pi32(float a)
{
    float m = fmodf(a, kTwoPi);
    if (m != 0.0f && m < 0.0f) m = __fadd_rn(m, kTwoPi);
    return m;
}
// np.linalg.norm of a float32 2-vector: sqrt of the dot product, no FMA
__device__ __forceinline__ float norm32(float dx, float dy) { return sqrtf(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy))); }
__device__ __forceinline__ float sign32(float v) { return v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : 0.0f); }

// What the steer needs beside the states: geometry, map and bounds travel in the library's SolveParams, so that the transit and
// the lookups are the library's own (mppi_geometry.h, mppi_chain.h).
struct ClrrtCommon {
    SolveParams p;
    int max_seqs;
    double delta, pid_dt;      // delta_distance; the PID's delta_t (the transit's is p.dt)
};

struct SteerOut {
    int feasible, length, word, npts;
    float cost, x, y, th;                  // the accumulated cost; the last state
    double e_lin, e_ang;                   // the controllers' previous errors
    float i_lin, i_ang;                    // ... and integrals
};

struct DubinsWord { float len, b0, b1, third; };

// The shortest of the six words (the first of equal lengths) from (sx, sy, sth) to (ex, ey, eth): dubins.py all_options, float32.
// Every lane evaluates the same values.  (lsx, lsy) / (rsx, rsy): the turning centres left / right of the start; le / re: of the end.
__device__ __forceinline__ int dubins_shortest(float sth, float eth, float lsx, float lsy, float rsx, float rsy, float lex, float ley,
                                               float rex, float rey, DubinsWord &best)
{
    const float inf = INFINITY;
    DubinsWord w;
    int word = 0;
    // LSL (ls -> le) and RSR (rs -> re); their centre distance and bearing serve LRL and RLR too
    const float dLx = __fsub_rn(lex, lsx), dLy = __fsub_rn(ley, lsy), dRx = __fsub_rn(rex, rsx), dRy = __fsub_rn(rey, rsy);
    const float nL = norm32(__fsub_rn(lsx, lex), __fsub_rn(lsy, ley)), nR = norm32(__fsub_rn(rsx, rex), __fsub_rn(rsy, rey));
    const float aL = atan2_32(dLy, dLx), aR = atan2_32(dRy, dRx);
    {
        const float b2 = mod2pi32(__fsub_rn(eth, aL)), b0 = mod2pi32(__fsub_rn(aL, sth));
        best = DubinsWord{__fadd_rn(__fadd_rn(b2, b0), nL), b0, b2, nL};
    }
    {
        const float b2 = mod2pi32(__fadd_rn(-eth, aR)), b0 = mod2pi32(__fadd_rn(-aR, sth));
        w = DubinsWord{__fadd_rn(__fadd_rn(b2, b0), nR), -b0, -b2, nR};
        if (w.len < best.len) { best = w; word = 1; }
    }
    // RSL (rs -> le), LSR (ls -> re)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float mx = __fmul_rn(__fsub_rn(k == 0 ? lex : rex, k == 0 ? rsx : lsx), 0.5f);
        const float my = __fmul_rn(__fsub_rn(k == 0 ? ley : rey, k == 0 ? rsy : lsy), 0.5f);
        const float psia = atan2_32(my, mx), half = norm32(mx, my);
        w.len = inf;
        if (!(half < 1.0f)) {
            const float al = (float)acos((double)__fdiv_rn(1.0f, half));
            float b0, b2;
            if (k == 0) {
                b0 = mod2pi32(-__fsub_rn(__fsub_rn(__fadd_rn(psia, al), sth), kHalfPi32));
                b2 = mod2pi32(__fsub_rn(__fsub_rn(__fsub_rn(__fadd_rn(kPi, eth), kHalfPi32), al), psia));
            } else {
                b0 = mod2pi32(__fadd_rn(__fsub_rn(__fsub_rn(psia, al), sth), kHalfPi32));
                b2 = mod2pi32(__fadd_rn(__fsub_rn(__fsub_rn(kHalfPi32, eth), al), psia));
            }
            const float sd = __fmul_rn(2.0f, sqrtf(__fsub_rn(__fmul_rn(half, half), 1.0f)));
            w = DubinsWord{__fadd_rn(__fadd_rn(b0, b2), sd), k == 0 ? -b0 : b0, k == 0 ? b2 : -b2, sd};
        }
        if (w.len < best.len) { best = w; word = 2 + k; }
    }
    // RLR (rs, re), LRL (ls, le)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float d = k == 0 ? nR : nL, at = k == 0 ? aR : aL;
        w.len = inf;
        if (!(d > 4.0f || d < 2.0f)) {
            const float gam = __fmul_rn(2.0f, (float)asin((double)__fdiv_rn(d, 4.0f)));
            const float tail = __fmul_rn(__fsub_rn(kPi, gam), 0.5f);
            float b0, b2;
            if (k == 0) {
                b0 = mod2pi32(__fadd_rn(__fadd_rn(__fadd_rn(-at, sth), kHalfPi32), tail));
                b2 = mod2pi32(__fadd_rn(__fadd_rn(__fsub_rn(at, eth), kHalfPi32), tail));
            } else {
                b0 = mod2pi32(__fadd_rn(__fadd_rn(__fsub_rn(at, sth), kHalfPi32), tail));
                b2 = mod2pi32(__fadd_rn(__fadd_rn(__fadd_rn(-at, eth), kHalfPi32), tail));
            }
            const float third = __fsub_rn(kTwoPi, gam);
            w = DubinsWord{__fadd_rn(__fadd_rn(third, fabsf(b0)), fabsf(b2)), k == 0 ? -b0 : b0, k == 0 ? -b2 : b2, third};
        }
        if (w.len < best.len) { best = w; word = 4 + k; }
    }
    return word;
}

// One _steer: Dubins path, truncation, closed-loop simulation.  Called by the whole wave with the same arguments; returns the same
// result in every lane.  lpts / lseg: 64 double2 / 64 double of LDS.  act (max_seqs, 2) and st (max_seqs + 1, 3) are this steer's
// rows in global memory (lane 0 writes).  RECORD: path (64, 2) float64 and tgt (max_seqs) receive the truncated path and the target
// index of every step.  The caller's next use of lpts / lseg must follow a barrier.
template <int GEO, bool RECORD>
__device__ SteerOut clrrt_steer(const ClrrtCommon &a, int b, float fx, float fy, float fth, float i_lin, float i_ang, float ex, float ey,
                                float eth, float gx, float gy, double2 *lpts, double *lseg, float *act, float *st, double *path_out,
                                int32_t *tgt_out)
{
    const SolveParams &p = a.p;
    const int lane = threadIdx.x;
    SteerOut r{};
    // ---- the word (dubins.py:79-114) ----
    float s1, c1, lsx, lsy, rsx, rsy, lex, ley, rex, rey;
    sincos32(__fadd_rn(fth, kHalfPi32), s1, c1); lsx = __fadd_rn(fx, c1); lsy = __fadd_rn(fy, s1);
    sincos32(__fadd_rn(fth, -kHalfPi32), s1, c1); rsx = __fadd_rn(fx, c1); rsy = __fadd_rn(fy, s1);
    sincos32(__fadd_rn(eth, kHalfPi32), s1, c1); lex = __fadd_rn(ex, c1); ley = __fadd_rn(ey, s1);
    sincos32(__fadd_rn(eth, -kHalfPi32), s1, c1); rex = __fadd_rn(ex, c1); rey = __fadd_rn(ey, s1);
    DubinsWord w;
    r.word = dubins_shortest(fth, eth, lsx, lsy, rsx, rsy, lex, ley, rex, rey, w);
    const bool straight = r.word < 4;
    // ---- generate_points_straight / _curve (dubins.py:348-425): the float32 constants of the chosen word ----
    const float a0 = fabsf(w.b0), a1 = fabsf(w.b1), sg0 = sign32(w.b0), sg1 = sign32(w.b1);
    const float c0x = w.b0 > 0.0f ? lsx : rsx, c0y = w.b0 > 0.0f ? lsy : rsy, c2x = w.b1 > 0.0f ? lex : rex, c2y = w.b1 > 0.0f ? ley : rey;
    float total, inix = fx, iniy = fy, finx = ex, finy = ey, dist = 1.0f, c1x = 0.0f, c1y = 0.0f, psi0 = 0.0f;
    if (straight) {
        total = __fadd_rn(__fadd_rn(a1, a0), w.third);
        if (a0 > 0.0f) {
            sincos32(__fadd_rn(fth, __fmul_rn(__fsub_rn(a0, kHalfPi32), sg0)), s1, c1);
            inix = __fadd_rn(c0x, c1); iniy = __fadd_rn(c0y, s1);
        }
        if (a1 > 0.0f) {
            sincos32(__fadd_rn(eth, __fmul_rn(__fsub_rn(-a1, kHalfPi32), sg1)), s1, c1);
            finx = __fadd_rn(c2x, c1); finy = __fadd_rn(c2y, s1);
        }
        dist = norm32(__fsub_rn(inix, finx), __fsub_rn(iniy, finy));
    } else {
        total = __fadd_rn(__fadd_rn(a1, a0), fabsf(w.third));
        const float inter = norm32(__fsub_rn(c0x, c2x), __fsub_rn(c0y, c2y));
        const float ux = __fdiv_rn(__fsub_rn(c2x, c0x), inter), uy = __fdiv_rn(__fsub_rn(c2y, c0y), inter);
        const float hi = __fmul_rn(inter, 0.5f);
        const float h = sqrtf(__fsub_rn(4.0f, __fmul_rn(hi, hi)));
        c1x = __fadd_rn(__fmul_rn(__fadd_rn(c0x, c2x), 0.5f), __fmul_rn(__fmul_rn(sg0, -uy), h));
        c1y = __fadd_rn(__fmul_rn(__fadd_rn(c0y, c2y), 0.5f), __fmul_rn(__fmul_rn(sg0, ux), h));
        psi0 = __fsub_rn(atan2_32(__fsub_rn(c1y, c0y), __fsub_rn(c1x, c0x)), kPi);
    }
    // ---- lane = point: arc length 0.25 lane; the end point follows the last of them ----
    const double count_d = ceil((double)total / 0.25);
    const int count = count_d < (double)kClrrtPoints ? max((int)count_d, 0) : kClrrtPoints;      // points before the end point, of those held
    const int ngen = min(count + 1, kClrrtPoints);
    double px = (double)ex, py = (double)ey;
    if (lane < count) {
        const double x = 0.25 * (double)lane, lim0 = (double)a0, lim1 = (double)__fsub_rn(total, a1);
        double ang = 0.0, cx = 0.0, cy = 0.0;
        bool arc = true;
        if (x < lim0) {
            ang = (double)fth + (x - kPi64 / 2) * (double)sg0; cx = (double)c0x; cy = (double)c0y;
        } else if (x > lim1) {
            ang = (double)eth + ((x - (double)total) - kPi64 / 2) * (double)sg1; cx = (double)c2x; cy = (double)c2y;
        } else if (straight) {
            arc = false;
            const double co = (x - (double)a0) / (double)dist;
            px = co * (double)finx + (1.0 - co) * (double)inix;
            py = co * (double)finy + (1.0 - co) * (double)iniy;
        } else {
            ang = (double)psi0 - (double)sg0 * (x - (double)a0); cx = (double)c1x; cy = (double)c1y;
        }
        if (arc) {
            double sd, cd;
            sincos(ang, &sd, &cd);
            px = cx + cd; py = cy + sd;
        }
    }
    lpts[lane] = make_double2(px, py);
    __syncthreads();
    // ---- truncation (cl_rrt.py:223-230): the first index whose sequential float64 cumulative length exceeds delta ----
    {
        double seg = 0.0;
        if (lane >= 1 && lane < ngen) {
            const double2 q = lpts[lane - 1];
            const double dx = px - q.x, dy = py - q.y;
            seg = sqrt(dx * dx + dy * dy);
        }
        lseg[lane] = seg;
    }
    __syncthreads();
    int npts = ngen;
    {
        double acc = 0.0;
        for (int i = 1; i < ngen; ++i) {
            acc += lseg[i];
            if (acc > a.delta) { npts = i; break; }
        }
    }
    r.npts = npts;
    if (RECORD && lane < kClrrtPoints) {
        path_out[2 * lane] = lane < npts ? px : NAN;
        path_out[2 * lane + 1] = lane < npts ? py : NAN;
    }
    const double2 last = lpts[npts - 1];
    // ---- _simulate_path_following (cl_rrt.py:249-315) ----
    const float *__restrict__ map = p.map + (size_t)b * p.map_stride;
    const Win win{0, 0, 0.f, 0.f, 0.f, 0.f};
    Chain c;
    c.x = fx; c.y = fy; c.th = fth;
    sincos_spec(c.th, c.sn, c.cs);
    c.trav = trav_lookup<GEO, false, true>(p, nullptr, map, win, c.x, c.y);
    if (lane == 0) { st[0] = fx; st[1] = fy; st[2] = fth; }
    float cost = 0.0f;
    double e_lin = 0.0, e_ang = 0.0;
    int t = 0;
    for (; t < a.max_seqs; ++t) {
        // PurePursuit._compute_target_points: the first point ahead (|bearing - heading| < pi / 2, not wrapped) beyond the look-ahead
        const double dx = px - (double)c.x, dy = py - (double)c.y;
        const double d2 = dx * dx + dy * dy;
        const double ang = atan2(dy, dx) - (double)c.th;
        const bool valid = lane < npts && fabs(ang) < kPi64 / 2 && d2 > 0.25;
        const unsigned long long mask = __ballot(valid);
        const int k = mask ? __ffsll((long long)mask) - 1 : npts - 1;
        // _calculate_errors on the target: the lane's own distance and bearing are the very expressions
        e_lin = sqrt(__shfl(d2, k, 64));
        double e = __shfl(ang, k, 64) + kPi64;
        double m = fmod(e, kTwoPi64);
        if (m != 0.0 && m < 0.0) m += kTwoPi64;
        e_ang = m - kPi64;
        // PIDController.update, kp = 1, ki = kd = 0: the control is the error; the float32 integral takes a float64 sum
        i_lin = (float)((double)i_lin + e_lin * a.pid_dt);
        i_ang = (float)((double)i_ang + e_ang * a.pid_dt);
        const float v = (float)e_lin, om = (float)e_ang;
        // transit (in place: slot t keeps the un-clamped, un-wrapped next state) and the stage cost at that slot
        float xn, yn, tn;
        chain_step<GEO, false, true, true, false, 0, true>(p, nullptr, map, win, c, clampf(v, p.umin0, p.umax0), clampf(om, p.umin1, p.umax1), xn, yn, tn);
        const float gdx = xn - gx, gdy = yn - gy;
        cost = cost + (sqrt_cr(gdx * gdx + gdy * gdy) + (c.trav <= p.thr ? 1.0e4f : 0.0f));
        if (lane == 0) {
            act[2 * t] = v; act[2 * t + 1] = om;
            st[3 * t] = xn; st[3 * t + 1] = yn; st[3 * t + 2] = tn;
            st[3 * t + 3] = c.x; st[3 * t + 4] = c.y; st[3 * t + 5] = c.th;
            if (RECORD) tgt_out[t] = k;
        }
        const double fxe = last.x - (double)c.x, fye = last.y - (double)c.y;
        if (sqrt(fxe * fxe + fye * fye) < 1.0) { r.feasible = 1; ++t; break; }
    }
    {
        const float gdx = c.x - gx, gdy = c.y - gy;
        cost = cost + (sqrt_cr(gdx * gdx + gdy * gdy) + (c.trav <= p.thr ? 1.0e4f : 0.0f));
    }
    r.length = t;
    r.cost = cost; r.x = c.x; r.y = c.y; r.th = c.th;
    r.e_lin = e_lin; r.e_ang = e_ang; r.i_lin = i_lin; r.i_ang = i_ang;
    return r;
}

struct ClrrtGrowArgs {
    ClrrtCommon c;
    const float *starts;       // (B, 3)
    const float *goals;        // (B, 3): the costs run against (x, y)
    const float *samples;      // (B, iters, 3)
    float *nodes;              // (B, cap, 3)
    int32_t *edges;            // (B, cap)
    float *costs;              // (B, cap)
    int32_t *seq_lengths;      // (B, cap)
    float *ctrl;               // (B, cap, 4)
    float *action_seqs;        // (B, cap, max_seqs, 2)
    float *state_seqs;         // (B, cap, max_seqs + 1, 3)
    int32_t *counts;           // (B)
    int32_t *near;             // (B, iters) nearest index of every iteration
    int32_t *feasible;         // (B, iters)
    int iters, cap;
    const int32_t *active;     // (B) or nullptr = every instance
};

template <int GEO>
__global__ __launch_bounds__(kClrrtThreads) void clrrt_grow_kernel(ClrrtGrowArgs a)
{
    extern __shared__ float2 lxy[];                        // cap (x, y), then cap (heading, cost, linear integral, angular integral)
    __shared__ double2 lpts[kClrrtPoints];
    __shared__ double lseg[kClrrtPoints];
    const int b = blockIdx.x, t = threadIdx.x, S = a.c.max_seqs;
    if (a.active && a.active[b] == 0) return;
    float4 *laux = (float4 *)(lxy + ((a.cap + 1) & ~1));          // 16-byte aligned behind the (x, y) pairs
    float *nodes = a.nodes + (size_t)b * a.cap * 3;
    int32_t *edges = a.edges + (size_t)b * a.cap, *lens = a.seq_lengths + (size_t)b * a.cap;
    float *costs = a.costs + (size_t)b * a.cap, *ctrl = a.ctrl + (size_t)b * a.cap * 4;
    float *aseq = a.action_seqs + (size_t)b * a.cap * S * 2, *sseq = a.state_seqs + (size_t)b * a.cap * (S + 1) * 3;
    const float *samp = a.samples + (size_t)b * a.iters * 3;
    const float gx = a.goals[3 * b], gy = a.goals[3 * b + 1];
    if (t == 0) {
        const float x = a.starts[3 * b], y = a.starts[3 * b + 1], th = a.starts[3 * b + 2];
        nodes[0] = x; nodes[1] = y; nodes[2] = th;
        edges[0] = -1; costs[0] = 0.0f; lens[0] = 0;
        ctrl[0] = ctrl[1] = ctrl[2] = ctrl[3] = 0.0f;
        lxy[0] = make_float2(x, y);
        laux[0] = make_float4(th, 0.0f, 0.0f, 0.0f);
    }
    for (int i = t; i < S * 2; i += kClrrtThreads) aseq[i] = 0.0f;                 // the root has no segment
    for (int i = t; i < (S + 1) * 3; i += kClrrtThreads) sseq[i] = 0.0f;
    __syncthreads();
    int n = 1;
    for (int it = 0; it < a.iters; ++it) {
        const float sx = samp[3 * it], sy = samp[3 * it + 1], sth = samp[3 * it + 2];
        unsigned long long key = ~0ull;
        for (int i = t; i < n; i += kClrrtThreads) {
            const float2 q = lxy[i];
            const float d = rrt_norm(__fsub_rn(q.x, sx), __fsub_rn(q.y, sy));
            const unsigned long long k = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)i;
            key = k < key ? k : key;
        }
        key = block_min_u64<kClrrtThreads>(key, nullptr);
        const int par = min((int)(unsigned)(key & 0xffffffffu), n - 1);
        const float2 f = lxy[par];
        const float4 fa = laux[par];
        float *act = aseq + (size_t)n * S * 2, *st = sseq + (size_t)n * (S + 1) * 3;
        // the root starts from zeroed controllers; any other node from its stored row, whose integrals the steer updates IN PLACE
        const SteerOut r = clrrt_steer<GEO, false>(a.c, b, f.x, f.y, fa.x, par ? fa.z : 0.0f, par ? fa.w : 0.0f, sx, sy, sth, gx, gy, lpts, lseg, act, st,
                                                   nullptr, nullptr);
        __syncthreads();
        if (t == 0) {
            a.near[(size_t)b * a.iters + it] = par;
            a.feasible[(size_t)b * a.iters + it] = r.feasible;
            if (par) {
                laux[par].z = r.i_lin; laux[par].w = r.i_ang;
                ctrl[4 * par + 1] = r.i_lin; ctrl[4 * par + 3] = r.i_ang;
            }
        }
        if (r.feasible) {
            // behind the segment the rows are zero, as the reference's: an earlier steer into this slot (an infeasible one of this plan, or
            // any of the handle's previous plan) may have written further
            for (int i = 2 * r.length + t; i < 2 * S; i += kClrrtThreads) act[i] = 0.0f;
            for (int i = 3 * (r.length + 1) + t; i < 3 * (S + 1); i += kClrrtThreads) st[i] = 0.0f;
            if (t == 0) {
                nodes[3 * n] = r.x; nodes[3 * n + 1] = r.y; nodes[3 * n + 2] = r.th;
                edges[n] = par; lens[n] = r.length;
                const float cn = __fadd_rn(laux[par].y, r.cost);
                costs[n] = cn;
                ctrl[4 * n] = (float)r.e_lin; ctrl[4 * n + 1] = r.i_lin; ctrl[4 * n + 2] = (float)r.e_ang; ctrl[4 * n + 3] = r.i_ang;
                lxy[n] = make_float2(r.x, r.y);
                laux[n] = make_float4(r.th, cn, r.i_lin, r.i_ang);
            }
            ++n;
        }
        __syncthreads();
    }
    if (t == 0) a.counts[b] = n;
}

struct ClrrtSteerArgs {
    ClrrtCommon c;
    const float *from;         // (B, 3)
    const float *ctrl;         // (B, 4): previous error and integral, linear then angular
    const float *targets;      // (B, 3)
    const float *goal;         // (2) the costs' goal
    float *actions;            // (B, max_seqs, 2)
    float *states;             // (B, max_seqs + 1, 3)
    double *paths;             // (B, 64, 2) NaN beyond the truncated path
    int32_t *tgt;              // (B, max_seqs)
    int32_t *results;          // (B, kClrrtSteerResult)
    float *cost;               // (B)
    double *ctrl_out;          // (B, 4)
};

template <int GEO>
__global__ __launch_bounds__(kClrrtThreads) void clrrt_steer_kernel(ClrrtSteerArgs a)
{
    __shared__ double2 lpts[kClrrtPoints];
    __shared__ double lseg[kClrrtPoints];
    const int b = blockIdx.x, t = threadIdx.x, S = a.c.max_seqs;
    const float *f = a.from + 3 * b, *cs = a.ctrl + 4 * b, *tg = a.targets + 3 * b;
    const SteerOut r = clrrt_steer<GEO, true>(a.c, b, f[0], f[1], f[2], cs[1], cs[3], tg[0], tg[1], tg[2], a.goal[0], a.goal[1], lpts, lseg,
                                              a.actions + (size_t)b * S * 2, a.states + (size_t)b * (S + 1) * 3, a.paths + (size_t)b * kClrrtPoints * 2,
                                              a.tgt + (size_t)b * S);
    if (t == 0) {
        int32_t *res = a.results + (size_t)b * kClrrtSteerResult;
        res[0] = r.feasible; res[1] = r.length; res[2] = r.word; res[3] = r.npts;
        a.cost[b] = r.cost;
        double *co = a.ctrl_out + 4 * b;
        co[0] = r.e_lin; co[1] = (double)r.i_lin; co[2] = r.e_ang; co[3] = (double)r.i_ang;
    }
}

struct ClrrtPathArgs {
    const float *nodes;
    const int32_t *edges;
    const float *costs;
    const int32_t *seq_lengths;
    const float *action_seqs, *state_seqs;
    const int32_t *counts;
    const float *goals;        // (B, 3)
    float *path_actions;       // (B, path_cap, 2), NaN beyond the path
    float *path_states;        // (B, path_cap + 1, 3)
    int32_t *results;          // (B, kClrrtResult)
    int cap, path_cap, max_seqs;
    float threshold;
    const int32_t *active;     // (B) or nullptr = every instance
};

__global__ __launch_bounds__(kClrrtPathThreads) void clrrt_path_kernel(ClrrtPathArgs a)
{
    __shared__ int sh[3];                                   // pick, total length, fits
    const int b = blockIdx.x, t = threadIdx.x, S = a.max_seqs;
    if (a.active && a.active[b] == 0) return;
    const float *nodes = a.nodes + (size_t)b * a.cap * 3, *costs = a.costs + (size_t)b * a.cap;
    const int32_t *edges = a.edges + (size_t)b * a.cap, *lens = a.seq_lengths + (size_t)b * a.cap;
    const float *aseq = a.action_seqs + (size_t)b * a.cap * S * 2, *sseq = a.state_seqs + (size_t)b * a.cap * (S + 1) * 3;
    float *pa = a.path_actions + (size_t)b * a.path_cap * 2, *ps = a.path_states + (size_t)b * (a.path_cap + 1) * 3;
    const int n = min(max(a.counts[b], 1), a.cap);
    const NearGoal g = near_goal_pick<3, kClrrtPathThreads>(nodes, costs, n, a.goals[3 * b], a.goals[3 * b + 1], a.threshold);
    if (t == 0) {
        const int total = g.total;
        int32_t *res = a.results + (size_t)b * kClrrtResult;
        int L = 0, pick = -1, fits = 1;
        if (total > 0) {
            pick = min((int)(unsigned)(g.key & 0xffffffffu), n - 1);
            int hops = 0;
            for (int cur = pick; cur != 0 && hops < n; ++hops) {                      // a parent has a lower index than its child
                L += min(max(lens[cur], 0), S);
                cur = min(max(edges[cur], 0), n - 1);
            }
            fits = L <= a.path_cap;
        }
        res[0] = total > 0; res[1] = pick; res[2] = L; res[3] = total; res[4] = fits ? BN_OK : BN_ERR_STATE; res[5] = n;
        sh[0] = pick; sh[1] = L; sh[2] = fits;
    }
    __syncthreads();
    const int pick = sh[0], fits = sh[2], L = (pick >= 0 && fits) ? sh[1] : 0;
    // _reconstruct_state_action_seq: the picked node's segment whole, every segment before it without its first state
    if (pick > 0 && fits) {
        int off = L, hops = 0;
        for (int cur = pick; cur != 0 && hops < n; ++hops) {
            const int len = min(max(lens[cur], 0), S);
            off -= len;
            const float *sa = aseq + (size_t)cur * S * 2, *ss = sseq + (size_t)cur * (S + 1) * 3;
            for (int i = t; i < 2 * len; i += kClrrtPathThreads) pa[2 * off + i] = sa[i];
            if (cur == pick) {
                for (int i = t; i < 3 * (len + 1); i += kClrrtPathThreads) ps[3 * off + i] = ss[i];
            } else {
                for (int i = t; i < 3 * len; i += kClrrtPathThreads) ps[3 * off + i] = ss[3 + i];
            }
            cur = min(max(edges[cur], 0), n - 1);
        }
    }
    const int rows = pick > 0 && fits ? L + 1 : 0;
    for (int i = 2 * L + t; i < 2 * a.path_cap; i += kClrrtPathThreads) pa[i] = NAN;
    for (int i = 3 * rows + t; i < 3 * (a.path_cap + 1); i += kClrrtPathThreads) ps[i] = NAN;
}

// A new episode of the plan-follow-replan loop: every instance's stream seeded as constructing its planner does, nothing drawn.
__global__ void clrrt_seed_kernel(const uint64_t *seeds, uint32_t *state, int32_t *pos, int B)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    mt_seed(state + (size_t)b * kMtN, (uint32_t)seeds[b]);
    pos[b] = kMtN;
}

thread_local std::string g_clrrt_error;

}  // namespace
}  // namespace bn

struct bn_clrrt {
    bn_clrrt_config cfg{};
    bn::ClrrtCommon c{};
    int B = 0, iters = 0, cap = 0, path_cap = 0, S = 0, geo = 0;
    bool seeded = false, ev_recorded = false, have_map = false;
    size_t lds_bytes = 0;
    bn::DeviceBuffers bufs;                  // every device pointer below, filled by bn_clrrt_create
    bn::DeviceBuffers late;                  // ... but inst_maps: built by the first bn_clrrt_set_instance_maps
    float *map = nullptr, *goal = nullptr;
    float *inst_maps = nullptr;              // (B, G, G) one risk map per instance; c.p.map points here while c.p.map_stride == G * G
    float *nodes = nullptr, *costs = nullptr, *ctrl = nullptr, *aseq = nullptr, *sseq = nullptr, *samples = nullptr, *starts = nullptr, *goals = nullptr;
    float *path_actions = nullptr, *path_states = nullptr;
    int32_t *edges = nullptr, *lens = nullptr, *counts = nullptr, *flags = nullptr, *results = nullptr, *pos = nullptr, *near = nullptr, *feasible = nullptr;
    uint32_t *state = nullptr;
    uint64_t *seeds = nullptr;
    // the steer without a tree
    float *st_from = nullptr, *st_ctrl = nullptr, *st_targets = nullptr, *st_actions = nullptr, *st_states = nullptr, *st_cost = nullptr;
    double *st_paths = nullptr, *st_ctrl_out = nullptr;
    int32_t *st_tgt = nullptr, *st_results = nullptr;
    unsigned char *pinned = nullptr;         // staging: 10 floats per instance, then a uint64 per instance
    uint64_t *pinned_seeds = nullptr;        // ... the seeds in it
    hipEvent_t ev_done = nullptr;
};

namespace {

int clrrt_fail(int code, const std::string &msg)
{
    bn::g_clrrt_error = msg;
    return code;
}

#define CLRRT_HIP(expr) BN_HIP_AS(clrrt_fail, expr, #expr)

bool clrrt_pow2(double v)
{
    int e = 0;
    return v > 0.0 && std::frexp(v, &e) == 0.5;
}

int clrrt_grow_and_pick(bn_clrrt_t *h, hipStream_t s, const int32_t *active = nullptr)
{
    bn::ClrrtGrowArgs g{};
    g.c = h->c; g.starts = h->starts; g.goals = h->goals; g.samples = h->samples; g.nodes = h->nodes; g.edges = h->edges; g.costs = h->costs;
    g.seq_lengths = h->lens; g.ctrl = h->ctrl; g.action_seqs = h->aseq; g.state_seqs = h->sseq; g.counts = h->counts; g.near = h->near;
    g.feasible = h->feasible; g.iters = h->iters; g.cap = h->cap; g.active = active;
    if (h->geo == bn::kGeoPow2) bn::clrrt_grow_kernel<bn::kGeoPow2><<<h->B, bn::kClrrtThreads, h->lds_bytes, s>>>(g);
    else bn::clrrt_grow_kernel<bn::kGeoPow2Origin0><<<h->B, bn::kClrrtThreads, h->lds_bytes, s>>>(g);
    CLRRT_HIP(hipGetLastError());
    bn::ClrrtPathArgs p{};
    p.nodes = h->nodes; p.edges = h->edges; p.costs = h->costs; p.seq_lengths = h->lens; p.action_seqs = h->aseq; p.state_seqs = h->sseq;
    p.counts = h->counts; p.goals = h->goals; p.path_actions = h->path_actions; p.path_states = h->path_states; p.results = h->results;
    p.cap = h->cap; p.path_cap = h->path_cap; p.max_seqs = h->S; p.threshold = (float)h->cfg.goal_threshold; p.active = active;
    bn::clrrt_path_kernel<<<h->B, bn::kClrrtPathThreads, 0, s>>>(p);
    CLRRT_HIP(hipGetLastError());
    return bn::tree_mark_done(h, s, clrrt_fail);
}

}  // namespace

// ---- what the plan-follow-replan loop drives (clrrt_view.h) ----
namespace bn {

int clrrt_view(bn_clrrt *h, ClrrtView *v)
{
    if (!h || !v) return clrrt_fail(BN_ERR_INVALID, "null argument");
    v->cfg = h->cfg; v->device = h->cfg.device_id; v->B = h->B; v->iters = h->iters; v->path_cap = h->path_cap; v->have_map = h->have_map;
    v->starts = h->starts; v->goals = h->goals; v->samples = h->samples; v->path_actions = h->path_actions; v->path_states = h->path_states;
    v->results = h->results;
    return BN_OK;
}

int clrrt_loop_reset(bn_clrrt *h, hipStream_t s, const float *goal_nodes, const uint64_t *seeds)
{
    if (!h || !goal_nodes || !seeds) return clrrt_fail(BN_ERR_INVALID, "null argument");
    for (int b = 0; b < h->B; ++b) {
        if (seeds[b] > 0xFFFFFFFFull) return clrrt_fail(BN_ERR_INVALID, "Seed must be between 0 and 2**32 - 1");
        if (!std::isfinite(goal_nodes[3 * b]) || !std::isfinite(goal_nodes[3 * b + 1]) || !std::isfinite(goal_nodes[3 * b + 2]))
            return clrrt_fail(BN_ERR_INVALID, "goal nodes must be finite");
    }
    BN_ON_DEVICE(clrrt_fail, h->cfg.device_id);
    if (h->ev_recorded) CLRRT_HIP(hipEventSynchronize(h->ev_done));                    // the staging block is free again
    const size_t B = h->B;
    std::memcpy(h->pinned + B * 12, goal_nodes, B * 12);
    uint64_t *ps = (uint64_t *)(h->pinned + B * 40);
    for (size_t b = 0; b < B; ++b) ps[b] = seeds[b];
    CLRRT_HIP(hipMemcpyAsync(h->goals, h->pinned + B * 12, B * 12, hipMemcpyHostToDevice, s));
    CLRRT_HIP(hipMemcpyAsync(h->seeds, ps, B * 8, hipMemcpyHostToDevice, s));
    clrrt_seed_kernel<<<(h->B + 63) / 64, 64, 0, s>>>(h->seeds, h->state, h->pos, h->B);
    CLRRT_HIP(hipGetLastError());
    if (int rc = tree_mark_done(h, s, clrrt_fail)) return rc;
    h->seeded = true;
    return BN_OK;
}

int clrrt_plan_masked(bn_clrrt *h, hipStream_t s, const int32_t *active, int draw)
{
    if (!h || !active) return clrrt_fail(BN_ERR_INVALID, "null argument");
    if (!h->have_map) return clrrt_fail(BN_ERR_STATE, "bn_clrrt_set_map has not been called");
    BN_ON_DEVICE(clrrt_fail, h->cfg.device_id);
    if (draw)
        if (int rc = tree_draw_samples<3>(h, s, false, active, clrrt_fail)) return rc;
    return clrrt_grow_and_pick(h, s, active);
}

}  // namespace bn

extern "C" {

const char *bn_clrrt_last_error(void) { return bn::g_clrrt_error.c_str(); }

void bn_clrrt_config_init(bn_clrrt_config *cfg)
{
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = (uint32_t)sizeof(*cfg);
    cfg->num_instances = 1;
    cfg->max_iterations = 500;               // cl_rrt.py:34-38
    cfg->max_seqs = 250;
    cfg->path_cap = 0;                       // 0: min(max_iterations * max_seqs, 65536)
    cfg->grid_size = 64;
    cfg->resolution = 0.5;
    cfg->x_limits[0] = 0.0; cfg->x_limits[1] = 32.0;
    cfg->y_limits[0] = 0.0; cfg->y_limits[1] = 32.0;
    cfg->delta_distance = 5.0;
    cfg->goal_sample_rate = 0.25;
    cfg->goal_threshold = 1.0;
    cfg->delta_t = 0.1;
    cfg->transit_dt = 0.1;                   // UnicycleModel.transit's default: CLRRT does not pass its own
    cfg->u_min[0] = 0.0; cfg->u_min[1] = -1.0; cfg->u_max[0] = 1.0; cfg->u_max[1] = 1.0;      // robot_model.py:54-57
    cfg->seed = 42;
}

int bn_clrrt_create(const bn_clrrt_config *cfg, bn_clrrt_t **out)
{
    if (!out) return clrrt_fail(BN_ERR_INVALID, "null handle pointer");
    *out = nullptr;
    if (!cfg) return clrrt_fail(BN_ERR_INVALID, "null config");
    if (cfg->struct_size != sizeof(bn_clrrt_config)) return clrrt_fail(BN_ERR_INVALID, "bn_clrrt_config.struct_size does not match this library");
    if (cfg->num_instances < 1 || cfg->num_instances > (1 << 16)) return clrrt_fail(BN_ERR_INVALID, "num_instances must be in [1, 65536]");
    if (cfg->max_iterations < 1 || cfg->max_iterations > bn::kClrrtMaxNodes - 1)
        return clrrt_fail(BN_ERR_INVALID, "max_iterations must be in [1, 2047]: the tree's nodes live in LDS");
    if (cfg->max_seqs < 1 || cfg->max_seqs > 4096) return clrrt_fail(BN_ERR_INVALID, "max_seqs must be in [1, 4096]");
    const int64_t longest = (int64_t)cfg->max_iterations * cfg->max_seqs;
    if (cfg->path_cap < 0 || cfg->path_cap > longest) return clrrt_fail(BN_ERR_INVALID, "path_cap must be in [0, max_iterations * max_seqs]");
    if ((int64_t)cfg->num_instances * ((int64_t)cfg->max_iterations + 1) * ((int64_t)cfg->max_seqs + 1) * 20 > ((int64_t)1 << 32))
        return clrrt_fail(BN_ERR_INVALID, "num_instances * (max_iterations + 1) * (max_seqs + 1) sequences exceed 4 GiB");
    for (double v : {cfg->x_limits[0], cfg->x_limits[1], cfg->y_limits[0], cfg->y_limits[1], cfg->delta_distance, cfg->goal_sample_rate,
                     cfg->goal_threshold, cfg->delta_t, cfg->transit_dt, cfg->resolution, cfg->u_min[0], cfg->u_min[1], cfg->u_max[0], cfg->u_max[1]})
        if (!std::isfinite(v)) return clrrt_fail(BN_ERR_INVALID, "limits, distances, rates, time steps and action bounds must be finite");
    if (cfg->grid_size < 1 || cfg->grid_size > 8192) return clrrt_fail(BN_ERR_INVALID, "grid_size must be in [1, 8192]");
    if (!clrrt_pow2(cfg->resolution)) return clrrt_fail(BN_ERR_INVALID, "resolution must be a power of two (the cell index is then an exact multiply)");
    if (std::fabs((cfg->x_limits[1] - cfg->x_limits[0]) - cfg->grid_size * cfg->resolution) > 1e-6 * cfg->grid_size * cfg->resolution ||
        std::fabs((cfg->y_limits[1] - cfg->y_limits[0]) - cfg->grid_size * cfg->resolution) > 1e-6 * cfg->grid_size * cfg->resolution)
        return clrrt_fail(BN_ERR_INVALID, "limits must span grid_size * resolution");
    // a truncated path holds at most delta / (shortest chord of a 0.25 arc) + 2 points; 64 lanes hold them up to 12
    if (!(cfg->delta_distance > 0.0) || cfg->delta_distance > 12.0) return clrrt_fail(BN_ERR_INVALID, "delta_distance must be in (0, 12]: one wave holds the path");
    if (!(cfg->delta_t > 0.0) || !(cfg->transit_dt > 0.0)) return clrrt_fail(BN_ERR_INVALID, "time steps must be positive");
    if (!(cfg->u_min[0] <= cfg->u_max[0]) || !(cfg->u_min[1] <= cfg->u_max[1])) return clrrt_fail(BN_ERR_INVALID, "action bounds must be ordered");
    if (cfg->seed > 0xFFFFFFFFull) return clrrt_fail(BN_ERR_INVALID, "Seed must be between 0 and 2**32 - 1");
    if (int rc = bn::open_device(cfg->device_id, clrrt_fail)) return rc;
    BN_ON_DEVICE(clrrt_fail, cfg->device_id);
    auto *h = new bn_clrrt_t();
    h->cfg = *cfg;
    h->B = cfg->num_instances; h->iters = cfg->max_iterations; h->cap = h->iters + 1; h->S = cfg->max_seqs;
    h->path_cap = cfg->path_cap ? cfg->path_cap : (int)std::min<int64_t>(longest, 65536);
    h->lds_bytes = (size_t)((h->cap + 1) & ~1) * 8 + (size_t)h->cap * 16;
    h->geo = (cfg->x_limits[0] == 0.0 && cfg->y_limits[0] == 0.0) ? bn::kGeoPow2Origin0 : bn::kGeoPow2;
    bn::SolveParams &p = h->c.p;
    p.G = cfg->grid_size; p.B = h->B; p.T = h->S; p.K = 1;
    p.res = (float)cfg->resolution; p.inv_res = 1.0f / p.res; p.pow2 = 1;
    p.x0 = (float)cfg->x_limits[0]; p.y0 = (float)cfg->y_limits[0]; p.x_hi = (float)cfg->x_limits[1]; p.y_hi = (float)cfg->y_limits[1];
    p.dt = (float)cfg->transit_dt; p.thr = 0.0f;
    p.umin0 = (float)cfg->u_min[0]; p.umin1 = (float)cfg->u_min[1]; p.umax0 = (float)cfg->u_max[0]; p.umax1 = (float)cfg->u_max[1];
    p.ref_order = 1; p.wrap_near = 0; p.map_stride = 0;
    h->c.max_seqs = h->S; h->c.delta = cfg->delta_distance; h->c.pid_dt = cfg->delta_t;
    const size_t B = h->B, nc = B * h->cap, ni = B * h->iters, S = h->S;
    bn::DeviceBuffers &t = h->bufs;
    t.add(&h->map, (size_t)p.G * p.G * 4);
    t.add(&h->goal, 8);
    t.add(&h->nodes, nc * 12, BN_CLRRT_BUF_NODES);
    t.add(&h->edges, nc * 4, BN_CLRRT_BUF_EDGES);
    t.add(&h->costs, nc * 4, BN_CLRRT_BUF_COSTS);
    t.add(&h->lens, nc * 4, BN_CLRRT_BUF_SEQ_LENGTHS);
    t.add(&h->ctrl, nc * 16, BN_CLRRT_BUF_CONTROLLERS);
    t.add(&h->aseq, nc * S * 8, BN_CLRRT_BUF_ACTION_SEQS);
    t.add(&h->sseq, nc * (S + 1) * 12, BN_CLRRT_BUF_STATE_SEQS);
    t.add(&h->counts, B * 4, BN_CLRRT_BUF_COUNTS);
    t.add(&h->samples, ni * 12, BN_CLRRT_BUF_SAMPLES);
    t.add(&h->flags, ni * 4, BN_CLRRT_BUF_SAMPLE_FLAGS);
    t.add(&h->near, ni * 4, BN_CLRRT_BUF_NEAREST);
    t.add(&h->feasible, ni * 4, BN_CLRRT_BUF_FEASIBLE);
    t.add(&h->path_actions, B * h->path_cap * 8, BN_CLRRT_BUF_PATH_ACTIONS);
    t.add(&h->path_states, B * ((size_t)h->path_cap + 1) * 12, BN_CLRRT_BUF_PATH_STATES);
    t.add(&h->results, B * bn::kClrrtResult * 4, BN_CLRRT_BUF_RESULTS);
    t.add(&h->state, B * bn::kMtN * 4, BN_CLRRT_BUF_MT_STATE);
    t.add(&h->pos, B * 4, BN_CLRRT_BUF_MT_POS);
    t.add(&h->starts, B * 12);
    t.add(&h->goals, B * 12);
    t.add(&h->seeds, B * 8);
    t.add(&h->st_from, B * 12);
    t.add(&h->st_ctrl, B * 16);
    t.add(&h->st_targets, B * 12);
    t.add(&h->st_actions, B * S * 8, BN_CLRRT_BUF_STEER_ACTIONS);
    t.add(&h->st_states, B * (S + 1) * 12, BN_CLRRT_BUF_STEER_STATES);
    t.add(&h->st_cost, B * 4, BN_CLRRT_BUF_STEER_COSTS);
    t.add(&h->st_paths, B * bn::kClrrtPoints * 16, BN_CLRRT_BUF_STEER_PATHS);
    t.add(&h->st_ctrl_out, B * 32, BN_CLRRT_BUF_STEER_CONTROLLERS);
    t.add(&h->st_tgt, B * S * 4, BN_CLRRT_BUF_STEER_TARGETS);
    t.add(&h->st_results, B * bn::kClrrtSteerResult * 4, BN_CLRRT_BUF_STEER_RESULTS);
    t.add_pinned(&h->pinned, B * 48);
    t.add_event(&h->ev_done);
    if (int rc = t.alloc_all(clrrt_fail)) {
        bn_clrrt_destroy(h);                 // leaves the error text alone
        return rc;
    }
    p.map = h->map;
    h->pinned_seeds = (uint64_t *)(h->pinned + B * 40);
    *out = h;
    return BN_OK;
}

void bn_clrrt_destroy(bn_clrrt_t *h)
{
    if (!h) return;
    bn::DeviceGuard guard(h->cfg.device_id);
    if (h->ev_recorded && h->ev_done) (void)hipEventSynchronize(h->ev_done);
    h->bufs.free_all();
    h->late.free_all();
    delete h;
}

int bn_clrrt_set_map(bn_clrrt_t *h, const float *risk, const float *goal, double stuck_threshold)
{
    if (!h || !risk || !goal) return clrrt_fail(BN_ERR_INVALID, "null argument");
    if (!std::isfinite(stuck_threshold) || !std::isfinite(goal[0]) || !std::isfinite(goal[1])) return clrrt_fail(BN_ERR_INVALID, "goal and stuck threshold must be finite");
    BN_ON_DEVICE(clrrt_fail, h->cfg.device_id);
    if (h->ev_recorded) CLRRT_HIP(hipEventSynchronize(h->ev_done));
    CLRRT_HIP(hipMemcpy(h->map, risk, (size_t)h->c.p.G * h->c.p.G * 4, hipMemcpyHostToDevice));
    CLRRT_HIP(hipMemcpy(h->goal, goal, 8, hipMemcpyHostToDevice));
    h->c.p.map = h->map; h->c.p.map_stride = 0;                     // back from per-instance maps, if they were set
    h->c.p.thr = (float)stuck_threshold;
    h->have_map = true;
    return BN_OK;
}

int bn_clrrt_set_instance_maps(bn_clrrt_t *h, void *stream, const void *risks, int where, double stuck_threshold)
{
    if (!h || !risks) return clrrt_fail(BN_ERR_INVALID, "null argument");
    if (where != BN_MEM_HOST && where != BN_MEM_DEVICE) return clrrt_fail(BN_ERR_INVALID, "where must be BN_MEM_HOST or BN_MEM_DEVICE");
    if (!std::isfinite(stuck_threshold)) return clrrt_fail(BN_ERR_INVALID, "stuck threshold must be finite");
    BN_ON_DEVICE(clrrt_fail, h->cfg.device_id);
    hipStream_t s = (hipStream_t)stream;
    if (h->ev_recorded) CLRRT_HIP(hipEventSynchronize(h->ev_done));                    // no launch of the handle reads a map any more
    const size_t bytes = (size_t)h->B * h->c.p.G * h->c.p.G * 4;
    if (h->late.list.empty()) h->late.add(&h->inst_maps, bytes);
    if (!h->late.live) {
        if (int rc = h->late.ensure(clrrt_fail)) return rc;
        CLRRT_HIP(hipStreamSynchronize(nullptr));                                       // the zero fill ran on the null stream
    }
    if (where == BN_MEM_HOST) {
        CLRRT_HIP(hipMemcpyAsync(h->inst_maps, risks, bytes, hipMemcpyHostToDevice, s));
        CLRRT_HIP(hipStreamSynchronize(s));                                             // the caller's array is consumed before this returns
    } else {
        CLRRT_HIP(hipMemcpyAsync(h->inst_maps, risks, bytes, hipMemcpyDeviceToDevice, s));
    }
    // the pointer and the stride change together, and only with the B maps behind them: a non-zero stride over h->map reads out of bounds
    h->c.p.map = h->inst_maps; h->c.p.map_stride = h->c.p.G * h->c.p.G;
    h->c.p.thr = (float)stuck_threshold;
    h->have_map = true;
    return BN_OK;
}

int bn_clrrt_plan_async(bn_clrrt_t *h, void *stream, const float *starts, const float *goals, const uint64_t *seeds)
{
    if (!h || !starts || !goals) return clrrt_fail(BN_ERR_INVALID, "null argument");
    if (!h->have_map) return clrrt_fail(BN_ERR_STATE, "bn_clrrt_set_map has not been called");
    return bn::tree_plan<3>(h, stream, starts, goals, seeds, clrrt_fail, [](bn_clrrt_t *hh, hipStream_t s) { return clrrt_grow_and_pick(hh, s); });
}

int bn_clrrt_grow_from_samples_async(bn_clrrt_t *h, void *stream, const float *starts, const float *goals, const void *samples, int where)
{
    if (!h || !starts || !goals || !samples) return clrrt_fail(BN_ERR_INVALID, "null argument");
    if (where != BN_MEM_HOST && where != BN_MEM_DEVICE) return clrrt_fail(BN_ERR_INVALID, "where must be BN_MEM_HOST or BN_MEM_DEVICE");
    if (!h->have_map) return clrrt_fail(BN_ERR_STATE, "bn_clrrt_set_map has not been called");
    return bn::tree_grow_from_samples<3>(h, stream, starts, goals, samples, where, clrrt_fail,
                                         [](bn_clrrt_t *hh, hipStream_t s) { return clrrt_grow_and_pick(hh, s); });
}

int bn_clrrt_steer_async(bn_clrrt_t *h, void *stream, const float *from_states, const float *controller_states, const float *targets)
{
    if (!h || !from_states || !controller_states || !targets) return clrrt_fail(BN_ERR_INVALID, "null argument");
    if (!h->have_map) return clrrt_fail(BN_ERR_STATE, "bn_clrrt_set_map has not been called");
    for (int i = 0; i < h->B * 3; ++i)
        if (!std::isfinite(from_states[i]) || !std::isfinite(targets[i])) return clrrt_fail(BN_ERR_INVALID, "states and targets must be finite");
    for (int i = 0; i < h->B * 4; ++i)
        if (!std::isfinite(controller_states[i])) return clrrt_fail(BN_ERR_INVALID, "controller states must be finite");
    BN_ON_DEVICE(clrrt_fail, h->cfg.device_id);
    hipStream_t s = (hipStream_t)stream;
    if (h->ev_recorded) CLRRT_HIP(hipEventSynchronize(h->ev_done));
    const size_t B = h->B;
    std::memcpy(h->pinned, from_states, B * 12);
    std::memcpy(h->pinned + B * 12, targets, B * 12);
    std::memcpy(h->pinned + B * 24, controller_states, B * 16);
    CLRRT_HIP(hipMemcpyAsync(h->st_from, h->pinned, B * 12, hipMemcpyHostToDevice, s));
    CLRRT_HIP(hipMemcpyAsync(h->st_targets, h->pinned + B * 12, B * 12, hipMemcpyHostToDevice, s));
    CLRRT_HIP(hipMemcpyAsync(h->st_ctrl, h->pinned + B * 24, B * 16, hipMemcpyHostToDevice, s));
    bn::ClrrtSteerArgs a{};
    a.c = h->c; a.from = h->st_from; a.ctrl = h->st_ctrl; a.targets = h->st_targets; a.goal = h->goal; a.actions = h->st_actions;
    a.states = h->st_states; a.paths = h->st_paths; a.tgt = h->st_tgt; a.results = h->st_results; a.cost = h->st_cost; a.ctrl_out = h->st_ctrl_out;
    if (h->geo == bn::kGeoPow2) bn::clrrt_steer_kernel<bn::kGeoPow2><<<h->B, bn::kClrrtThreads, 0, s>>>(a);
    else bn::clrrt_steer_kernel<bn::kGeoPow2Origin0><<<h->B, bn::kClrrtThreads, 0, s>>>(a);
    CLRRT_HIP(hipGetLastError());
    return bn::tree_mark_done(h, s, clrrt_fail);
}

int bn_clrrt_sync(bn_clrrt_t *h)
{
    if (!h) return clrrt_fail(BN_ERR_INVALID, "null handle");
    BN_ON_DEVICE(clrrt_fail, h->cfg.device_id);
    return bn::tree_wait_done(h, clrrt_fail);
}

int bn_clrrt_device_buffer(bn_clrrt_t *h, int which, void **ptr, size_t *bytes)
{
    if (!h || !ptr || !bytes) return clrrt_fail(BN_ERR_INVALID, "null argument");
    if (!h->bufs.find(which, ptr, bytes)) return clrrt_fail(BN_ERR_INVALID, "unknown CL-RRT buffer id");
    return BN_OK;
}

int32_t bn_clrrt_path_cap(bn_clrrt_t *h) { return h ? h->path_cap : -1; }

}  // extern "C"
