// clrrt_loop.hip -- the follow half of the reference's CL-RRT driver loop (test/test_cl_rrt.py:167-200) on the device, for B rovers
// (DESIGN.md 4.8).  The planning half is the CL-RRT handle's own kernels (clrrt_kernels.hip) run under a mask; the host only looks
// at one counter between a round of replans and the next follow launch (bn_clrrt_loop_run, mppi_loops.cpp).
//
// clrrt_follow_kernel<GEO>: one workgroup of 256 threads per rover.  It runs the rover's loop iterations from the rover's own
// counter to the end of the call and stops early where the rover needs a plan: it then writes the rover's state into the planner's
// `starts` row, sets the rover's `active` word, adds one to `pending` and returns.  The launch after the masked plan takes the
// plan's result row (or a status: the reference raises or fails there) and goes on.  Per iteration, in the reference's order:
//   deviation   t > 0: min over ALL L + 1 planned states of rrt_norm(plan_xy - state_xy), float32 (torch.norm(..., dim=2) then
//               torch.min); > 1.0 flags a replan and the iteration takes no step.
//   action      plan_actions[action_index++]; action_index == L is the reference's IndexError: PLAN_EXHAUSTED.
//   env step    env_advance of mppi_env_step.h: observation-mode transit with the slip draw of iteration t (z row t of the call, or
//               Philox keyed by (env seed, t)), then the goal test, then the time limit on the rover's own step count.
// The steps of a rover depend on one another, so one iteration is one scan of the plan, ONE barrier and one env_advance: the
// threads stride over the planned (x, y) -- staged in LDS as float2 at launch when L + 1 <= kClrrtFollowLdsStates, else read from
// the path buffer -- the waves reduce with DPP, the four partial minima go through LDS slots that alternate with the iteration's
// parity (the slot written in iteration i is next written in i + 2, behind the barrier of i + 1 that every reader of i has
// passed), and the latent cell's two loads (env_fetch) are issued before the scan so that they are back behind the barrier.
// Every lane evaluates the step itself (same inputs, same operations); lane 0 logs.  min() is exact, so the LDS and the global
// path give the same bits.  Every loop is bounded by the call's iteration count; no workgroup waits for another.
//
// clrrt_outcome_kernel: behind a run, the rovers' words as bn_episode_score takes them (done_step, stopped) and as a campaign
// reads them (status, plans), one thread per rover.
#include "../../include/benchnav_mppi.h"
#include "clrrt_view.h"
#include "dwa_device.h"
#include "mppi_env_step.h"
#include "rollout_launch.h"
#include "rrt_device.h"

namespace bn {

namespace {

// row `row` of the call's logs for rover b (one lane); the state goes to row + 1
__device__ __forceinline__ void follow_log(const ClrrtFollowArgs &a, int row, int b, float x, float y, float th, float reward, float u0, float u1,
                                           float dev, int plan, int event)
{
    const size_t r = a.log.write(row, b, x, y, th, reward, u0, u1);
    a.log_dev[r] = dev;
    a.log_plan[r] = plan;
    a.log_event[r] = event;
}

template <int GEO>
__global__ __launch_bounds__(kClrrtFollowThreads) void clrrt_follow_kernel(const SolveParams p, const ClrrtFollowArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float2 lxy[];      // the plan's (x, y) pairs (use_lds)
    __shared__ float red[2][kClrrtFollowThreads / 64];
    const int tid = threadIdx.x, b = blockIdx.x;
    ClrrtRover r = a.rover[b];
    float sx = a.state[b * 3 + 0], sy = a.state[b * 3 + 1], sth = a.state[b * 3 + 2];
    const int end = a.iter0 + a.n;
    const float *pa = a.path_actions + (size_t)b * a.path_cap * 2;
    const float *ps = a.path_states + (size_t)b * ((size_t)a.path_cap + 1) * 3;
    int it = min(max(r.iter, a.iter0), end);
    if (it == a.iter0 && tid == 0) { a.log.states[b * 3 + 0] = sx; a.log.states[b * 3 + 1] = sy; a.log.states[b * 3 + 2] = sth; }
    // the plan the previous round asked for: CLRRT.forward's return, in its order (None, then _raise_unless_path)
    if (r.status == BN_CL_RUNNING && r.need == 2) {
        const int32_t *res = a.results + (size_t)b * kClrrtResultWords;
        ++r.plans;
        if (!res[0]) r.status = BN_CL_NO_PLAN;
        else if (res[4] != 0) r.status = BN_CL_PATH_OVERFLOW;
        else if (res[1] == 0) r.status = BN_CL_NO_SEQUENCE;
        else { r.length = min(max(res[2], 0), a.path_cap); r.aidx = 0; }
        r.need = 0;
        if (r.status != BN_CL_RUNNING) r.done_iter = it;
        if (tid == 0) a.active[b] = 0;
    }
    const int np = r.length + 1;
    const bool in_lds = a.use_lds && np <= kClrrtFollowLdsStates;
    if (in_lds && r.status == BN_CL_RUNNING && r.need == 0)
        for (int i = tid; i < np; i += kClrrtFollowThreads) lxy[i] = make_float2(ps[3 * i], ps[3 * i + 1]);
    __syncthreads();

    for (; it < end; ++it) {
        const int row = it - a.iter0;
        if (r.status == BN_CL_RUNNING && r.need == 1) {
            // forward's bounds test on the start and the goal node (cl_rrt.py), then the request
            const float gx = a.goal_nodes[3 * b], gy = a.goal_nodes[3 * b + 1];
            const bool in = a.xlo <= (double)sx && (double)sx <= a.xhi && a.ylo <= (double)sy && (double)sy <= a.yhi &&
                            a.xlo <= (double)gx && (double)gx <= a.xhi && a.ylo <= (double)gy && (double)gy <= a.yhi;
            if (!in) { r.status = BN_CL_OUT_OF_BOUNDS; r.done_iter = it; }
            else if (a.inj && r.plans >= a.P) { r.status = BN_CL_NO_PLAN; r.done_iter = it; }      // teacher forcing: no table left
            else {
                if (a.inj) {
                    const float *src = a.inj + ((size_t)r.plans * gridDim.x + b) * a.iters * 3;
                    float *dst = a.psamples + (size_t)b * a.iters * 3;
                    for (int i = tid; i < a.iters * 3; i += kClrrtFollowThreads) dst[i] = src[i];
                }
                if (tid == 0) {
                    a.starts[3 * b] = sx; a.starts[3 * b + 1] = sy; a.starts[3 * b + 2] = sth;
                    a.active[b] = 1;
                    atomicAdd(a.pending, 1);
                }
                r.need = 2;
                break;
            }
        }
        if (r.status != BN_CL_RUNNING) {                   // frozen: the state stays, the rest of the row is NaN
            if (tid == 0) follow_log(a, row, b, sx, sy, sth, NAN, NAN, NAN, NAN, r.plans - 1, BN_CL_EVENT_FROZEN);
            continue;
        }
        const EnvCell lc = env_fetch<GEO>(p, b, sx, sy);   // in flight across the scan and the barrier
        float dev = NAN;
        if (it > 0) {
            float m = INFINITY;
            if (in_lds) {
                for (int i = tid; i < np; i += kClrrtFollowThreads) {
                    const float2 q = lxy[i];
                    m = fminf(m, rrt_norm(__fsub_rn(q.x, sx), __fsub_rn(q.y, sy)));
                }
            } else {
                for (int i = tid; i < np; i += kClrrtFollowThreads)
                    m = fminf(m, rrt_norm(__fsub_rn(ps[3 * i], sx), __fsub_rn(ps[3 * i + 1], sy)));
            }
            m = -wave_max(-m);
            float *slot = red[it & 1];
            if ((tid & 63) == 0) slot[tid >> 6] = m;
            __syncthreads();
            dev = fminf(fminf(slot[0], slot[1]), fminf(slot[2], slot[3]));
            if (dev > 1.0f) {                              // is_replan: this iteration takes no step
                r.need = 1;
                if (tid == 0) follow_log(a, row, b, sx, sy, sth, NAN, NAN, NAN, dev, r.plans - 1, BN_CL_EVENT_REPLAN);
                continue;
            }
        }
        if (r.aidx >= r.length) {                          // action_seq[action_index]: the reference's IndexError
            r.status = BN_CL_PLAN_EXHAUSTED; r.done_iter = it;
            if (tid == 0) follow_log(a, row, b, sx, sy, sth, NAN, NAN, NAN, dev, r.plans - 1, BN_CL_EVENT_FROZEN);
            continue;
        }
        const float u0 = pa[2 * r.aidx], u1 = pa[2 * r.aidx + 1];
        ++r.aidx;
        const EnvStep e = env_advance_with<GEO>(p, b, sx, sy, sth, u0, u1, a.z ? a.z + (size_t)row * gridDim.x : nullptr, (uint64_t)it, lc);
        ++r.steps;
        sx = e.x; sy = e.y; sth = e.th;
        if (tid == 0) follow_log(a, row, b, sx, sy, sth, e.reward, u0, u1, dev, r.plans - 1, BN_CL_EVENT_STEP);
        if (e.reached) { r.status = BN_CL_GOAL; r.done_iter = it; }                                // is_terminated first
        else if (r.steps >= a.limit_steps) { r.status = BN_CL_TIME_LIMIT; r.done_iter = it; }      // elapsed > time_limit
    }
    r.iter = it;
    if (tid == 0) {
        a.rover[b] = r;
        a.state[b * 3 + 0] = sx; a.state[b * 3 + 1] = sy; a.state[b * 3 + 2] = sth;
    }
}

// The rovers' words as the episode scores read them (ClrrtOutcome, clrrt_view.h): one thread per rover, behind a run's last launch.
__global__ void clrrt_outcome_kernel(const ClrrtRover *__restrict__ rover, ClrrtOutcome out)
{
    const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= out.B) return;
    const ClrrtRover r = rover[b];
    const bool regular = r.status == BN_CL_RUNNING || r.status == BN_CL_GOAL || r.status == BN_CL_TIME_LIMIT;
    out.done_step()[b] = r.status == BN_CL_GOAL ? r.done_iter : -1;
    out.stopped()[b] = regular ? 0 : r.status;
    out.status()[b] = r.status;
    out.plans()[b] = r.plans;
}

template <int GEO>
hipError_t launch_g(const SolveParams &p, const ClrrtFollowArgs &a, hipStream_t s)
{
    const size_t lds = a.use_lds ? (size_t)kClrrtFollowLdsStates * sizeof(float2) : 0;
    hipError_t e = ensure_lds(clrrt_follow_kernel<GEO>, lds);
    if (e != hipSuccess) return e;
    clrrt_follow_kernel<GEO><<<dim3(p.B), dim3(kClrrtFollowThreads), lds, s>>>(p, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_clrrt_follow(const SolveParams &p, const ClrrtFollowArgs &a, hipStream_t s)
{
    switch (geo_of(p)) {
    case kGeoPow2Origin0: return launch_g<kGeoPow2Origin0>(p, a, s);
    case kGeoPow2: return launch_g<kGeoPow2>(p, a, s);
    default: return launch_g<kGeoGeneral>(p, a, s);
    }
}

hipError_t launch_clrrt_outcome(const ClrrtRover *rover, const ClrrtOutcome &out, hipStream_t s)
{
    clrrt_outcome_kernel<<<dim3((unsigned)((out.B + 63) / 64)), dim3(64), 0, s>>>(rover, out);
    return hipGetLastError();
}

}  // namespace bn
