// astar_dwa.hip -- the A* + DWA closed loop of the reference's test/test_astar_dwa.py:179-211 on the device, for B instances.
//
// One workgroup per instance (grid = B); instances are independent.  A workgroup loops over up to kAstarDwaStepsPerLaunch control
// steps; the host chains launches on one stream.  Each step, in the reference loop's order:
//   1. start cell   AStar._pos_to_index (astar.py:215-228): int((x - x_limits[0]) / res) in f32, TRUNCATED; the bounds test on the
//                   result (astar.py:88-92).  A failed test -- or a goal out of bounds / in collision (:93-94), or a failed A* solve --
//                   freezes the instance with a status code (the reference raises there).
//   2. path         the walk of the A* handle's next-hop map from the start cell to the goal (astar_kernels.hip; the reference's
//                   _reconstruct_path, :194-213: point = f32(ix) * f32(res), start included, x_limits[0] ignored).  An unreachable
//                   start is the reference's None, and DWA.update_reference_path(None) keeps the previous path: the walk from the
//                   instance's root cell (the last start whose walk reached the goal).  No root yet: the stage cost runs against the
//                   goal (dwa.py:243-247).
//   3. window + sub-goal, 4. rollouts + argmin: DWA.forward (dwa.py:116-153) with dwa_device.h, the code of the stand-alone kernels.
//   5. env step     PlanetaryEnv.step (planetary_env.py:189-219): env_advance of mppi_env_step.h with the argmin action.
// The path is never materialised: one lane chases `next` (staged in LDS when it fits) a segment of nthreads nodes at a time and
// the workgroup evaluates the segment's distances.  With the A* handle's jump tables (walk mode 1, JUMP) every lane fetches its
// own node of the segment instead, by pointer doubling: the same nodes in the same order, so the outputs are bit-identical.
// Pass 1 finds the nearest ahead distance over the whole path, pass 2 the first index at that distance (usually in the first
// segment: the sub-goal lies a look-ahead distance from the rover).
#include "../../include/benchnav_mppi.h"
#include "astar_dwa.h"
#include "dwa_device.h"
#include "mppi_env_step.h"
#include "rollout_launch.h"

namespace bn {

namespace {

// the reference's direction order (astar.py:154-163) as (dx, dy), two bits each (d + 1)
constexpr uint32_t kDirX = (0u << 0) | (2u << 2) | (1u << 4) | (1u << 6) | (0u << 8) | (0u << 10) | (2u << 12) | (2u << 14);
constexpr uint32_t kDirY = (1u << 0) | (1u << 2) | (0u << 4) | (2u << 6) | (0u << 8) | (2u << 10) | (0u << 12) | (2u << 14);
constexpr uint8_t kNextGoal = 8;

struct WalkSeg { int n, code, last; };   // nodes in the segment; 0 go on, 1 goal reached, 2 broken walk; the last node (iy * W + ix)

// Lane 0 appends up to nthreads nodes of the walk from *cur to seg (iy * W + ix each) and advances *cur; every lane gets the result.
// `total` = nodes walked before this segment.  A walk longer than H * W nodes (D strictly falls along next: impossible for a valid
// field) or onto a cell that has no next hop or off the map ends as broken.
__device__ __forceinline__ WalkSeg walk_segment(const uint8_t *nx, int W, int cells, int *cur, int total, int *seg, int *ctl,
                                                int tid, int nthreads)
{
    if (tid == 0) {
        int c = *cur, n = 0, code = 0;
        int iy = c / W, ix = c - iy * W;
        while (n < nthreads) {
            seg[n++] = c;
            const uint32_t h = nx[c];
            if (h == kNextGoal) { code = 1; break; }
            if (h > kNextGoal || total + n >= cells) { code = 2; break; }
            ix += (int)((kDirX >> (2 * h)) & 3u) - 1;
            iy += (int)((kDirY >> (2 * h)) & 3u) - 1;
            if (ix < 0 || ix >= W || iy < 0 || iy * W >= cells) { code = 2; break; }     // (not for a valid field)
            c = iy * W + ix;
        }
        ctl[0] = n; ctl[1] = code; ctl[2] = seg[n - 1]; ctl[3] = c;
    }
    __syncthreads();
    const WalkSeg r{ctl[0], ctl[1], ctl[2]};
    *cur = ctl[3];
    return r;
}

// The same segment through the jump tables: node total + t of the path is the segment's first cell advanced over the set bits
// of t, fetched by lane t itself.  *cur is the segment's first cell and *left the nodes of the path from it on (hops + 1; <= 0:
// the walk does not end at the goal, a broken walk as walk_segment reports one).  t < *left <= H W <= 2^levels, so every set bit
// of t is a kept level.  The next segment starts one hop past this one's last node.
__device__ __forceinline__ WalkSeg jump_segment(const int32_t *jump, int cells, int *cur, int *left, int *seg, int tid, int nthreads)
{
    const int first = *cur, rem = *left;
    if (rem <= 0) return WalkSeg{0, 2, first};
    const int n = rem < nthreads ? rem : nthreads;
    if (tid < n) {
        int c = first;
        for (int r = tid, lvl = 0; r; r >>= 1, ++lvl)
            if (r & 1) c = jump[(size_t)lvl * cells + c];
        seg[tid] = c;
    }
    __syncthreads();
    const int last = seg[n - 1];
    if (rem > nthreads) {
        *cur = jump[last];
        *left = rem - nthreads;
        return WalkSeg{n, 0, last};
    }
    return WalkSeg{n, 1, last};
}

// row gs of the call's logs for instance b (one lane)
__device__ __forceinline__ void log_step(const AstarDwaArgs &a, int gs, int b, float x, float y, float th, float reward, float u0, float u1,
                                         float hx, float hy)
{
    const size_t r = a.log.write(gs, b, x, y, th, reward, u0, u1);
    a.log_subgoal[r * 2 + 0] = hx; a.log_subgoal[r * 2 + 1] = hy;
}

// a frozen instance: the state stays, the rest of the row is NaN (the reference loop raised at or before this step)
__device__ __forceinline__ void log_frozen(const AstarDwaArgs &a, int gs, int b, float x, float y, float th)
{
    log_step(a, gs, b, x, y, th, NAN, NAN, NAN, NAN, NAN);
}

template <int GEO, bool LDSWIN, bool NEXT_LDS, bool JUMP>
__global__ void astar_dwa_kernel(const SolveParams p, const AstarDwaArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, nthreads = blockDim.x, b = blockIdx.x;
    const int NA = a.nv * a.nw, W = a.W, cells = a.H * a.W;
    float *win = smem;                                     // DWA's map window (LDSWIN)
    float *red = win + (LDSWIN ? p.WN * p.WN : 0);         // 16 floats + 16 ints
    int *redi = reinterpret_cast<int *>(red + 16);
    float *act = red + 32;                                 // (NA, 2) candidates
    int *seg = reinterpret_cast<int *>(act + 2 * NA);      // (nthreads) walk segment
    int *ctl = seg + nthreads;                             // 4 ints: the segment's summary
    uint8_t *nx_lds = reinterpret_cast<uint8_t *>(ctl + 4);   // (H, W) next-hop map (NEXT_LDS)

    const uint8_t *nx = a.next + (size_t)b * cells;
    if (NEXT_LDS) {
        if ((cells & 3) == 0 && ((reinterpret_cast<uintptr_t>(nx) & 3) == 0)) {
            const uint32_t *src = reinterpret_cast<const uint32_t *>(nx);
            uint32_t *dst = reinterpret_cast<uint32_t *>(nx_lds);
            for (int i = tid; i < cells / 4; i += nthreads) dst[i] = src[i];
        } else {
            for (int i = tid; i < cells; i += nthreads) nx_lds[i] = nx[i];
        }
        nx = nx_lds;                                       // (visible to lane 0's walk after the first barrier below)
    }

    float sx = a.state[b * 3 + 0], sy = a.state[b * 3 + 1], sth = a.state[b * 3 + 2];
    float pv = a.prev[b * 2 + 0], pw = a.prev[b * 2 + 1];
    int root = a.root[b], status = a.status[b], status_step = a.status_step[b], done = a.done[b];
    const float gx = p.goal[b * 2 + 0], gy = p.goal[b * 2 + 1];
    // the checks of AStar.forward that do not depend on the start (astar.py:88-94), in its order after a failed solve
    const AStarInst gi = a.ainst[b];
    int goal_code = BN_AD_OK;
    const int32_t *hops = JUMP ? a.hops + (size_t)b * cells : nullptr;
    const int32_t *jump = JUMP ? a.jump + (size_t)b * a.levels * cells : nullptr;
    if (*a.aerr != 0 || (JUMP && *a.jerr != 0)) goal_code = BN_AD_FIELD_ERROR;
    else if (gi.gx < 0) goal_code = BN_AD_OUT_OF_BOUNDS;
    else if (a.arisk[(size_t)b * cells + (size_t)gi.gy * W + gi.gx] <= gi.thr) goal_code = BN_AD_GOAL_COLLISION;
    const size_t B = p.B;
    if (a.s0 == 0 && tid == 0) { a.log.states[b * 3 + 0] = sx; a.log.states[b * 3 + 1] = sy; a.log.states[b * 3 + 2] = sth; }

    for (int i = 0; i < a.ns; ++i) {
        const int gs = a.s0 + i;                           // step of this call
        const uint64_t ep = a.step0 + (uint64_t)gs;        // step of the episode
        __syncthreads();                                   // the previous step's reads of act / win / red / seg are done
        int start = -1;
        if (status == BN_AD_OK) {
            // AStar._pos_to_index: int() truncates, so (-1, 0) is cell 0; NaN and anything at or past the edge fail the bounds test
            const float qx = (sx - p.x0) / p.res, qy = (sy - p.y0) / p.res;
            const bool in = qx > -1.0f && qx < (float)W && qy > -1.0f && qy < (float)a.H;
            if (goal_code == BN_AD_FIELD_ERROR) status = BN_AD_FIELD_ERROR;
            else if (!in || goal_code == BN_AD_OUT_OF_BOUNDS) status = BN_AD_OUT_OF_BOUNDS;   // "Start or goal position is out of bounds."
            else status = goal_code;                                                          // "Goal position is not traversable."
            if (status != BN_AD_OK) status_step = (int)ep;
            else start = (int)qy * W + (int)qx;
        }
        if (status != BN_AD_OK) {                          // frozen: the reference raised at or before this step
            if (tid == 0) log_frozen(a, gs, b, sx, sy, sth);
            continue;
        }
        const DwaWindow d = dwa_window(p, pv, pw, a.alim0, a.alim1, a.dwa_dt);
        dwa_window_actions(d, a.nv, a.nw, act, tid, nthreads);
        __syncthreads();                                   // (the LDS copy of next, on the first step)
        // the path: from the start cell, or -- unreachable, the reference's None -- the previous one, from the root cell
        const int origin = (JUMP ? hops[start] < 0 : nx[start] == 255) ? root : start;
        float hx = gx, hy = gy;                            // no path yet: the goal (dwa.py:243-247)
        if (origin >= 0) {
            float x, y, th;
            dwa_subgoal_state<GEO>(p, b, sx, sy, sth, d, a.nv, a.nw, x, y, th);
            // pass 1: the nearest ahead distance over the path, and the path's last point
            float best = INFINITY;
            int cur = origin, total = 0;
            const int nodes = JUMP ? hops[origin] + 1 : 0;     // of the whole path (JUMP)
            int left = nodes;
            WalkSeg ws;
            do {
                ws = JUMP ? jump_segment(jump, cells, &cur, &left, seg, tid, nthreads)
                          : walk_segment(nx, W, cells, &cur, total, seg, ctl, tid, nthreads);
                if (tid < ws.n) {
                    const int c = seg[tid], iy = c / W, ix = c - iy * W;
                    best = fminf(best, dwa_ahead_dist((float)ix * p.res, (float)iy * p.res, x, y, th, a.lookahead));
                }
                total += ws.n;
                __syncthreads();                           // seg / ctl are rewritten by the next segment
            } while (ws.code == 0);
            if (ws.code != 1) {                            // broken walk: the field is not a valid solve
                status = BN_AD_FIELD_ERROR;
                status_step = (int)ep;
                if (tid == 0) {
                    atomicOr(a.err, 1);
                    log_frozen(a, gs, b, sx, sy, sth);
                }
                continue;
            }
            if (origin == start) root = start;             // this walk reached the goal: the path DWA keeps from now on
            best = block_min(best, red, tid, nthreads);
            int pick = ws.last;                            // nothing ahead: the path's last point
            if (best < INFINITY) {
                // pass 2: the first index over ALL points at that distance (torch.where(distances == min)[0][0])
                cur = origin; total = 0; left = nodes;
                int found = 0x7fffffff;
                do {
                    __syncthreads();                       // redi of the previous segment's minimum has been read
                    ws = JUMP ? jump_segment(jump, cells, &cur, &left, seg, tid, nthreads)
                              : walk_segment(nx, W, cells, &cur, total, seg, ctl, tid, nthreads);
                    int idx = 0x7fffffff;
                    if (tid < ws.n) {
                        const int c = seg[tid], iy = c / W, ix = c - iy * W;
                        if (dwa_point_dist((float)ix * p.res, (float)iy * p.res, x, y) == best) idx = tid;
                    }
                    found = block_min_i(idx, redi, tid, nthreads);
                    if (found != 0x7fffffff) pick = seg[found];
                    total += ws.n;
                    __syncthreads();
                } while (found == 0x7fffffff && ws.code == 0);
            }
            const int piy = pick / W, pix = pick - piy * W;
            hx = (float)pix * p.res;
            hy = (float)piy * p.res;
        }
        const int imin = dwa_rollout_argmin<GEO, LDSWIN>(p, b, sx, sy, sth, act, NA, hx, hy, gx, gy, win, red, tid, nthreads,
                                                         nullptr, nullptr, nullptr);
        pv = act[imin * 2 + 0];                            // optimal_action_seq = actions[argmin]; the next window's centre (dwa.py:147)
        pw = act[imin * 2 + 1];
        const EnvStep e = env_advance<GEO>(p, b, sx, sy, sth, pv, pw, a.z ? a.z + (size_t)gs * B : nullptr, ep);
        if (tid == 0) log_step(a, gs, b, e.x, e.y, e.th, e.reward, pv, pw, hx, hy);
        if (e.reached && done < 0) done = (int)ep;
        sx = e.x; sy = e.y; sth = e.th;
    }
    if (tid == 0) {
        a.state[b * 3 + 0] = sx; a.state[b * 3 + 1] = sy; a.state[b * 3 + 2] = sth;
        a.prev[b * 2 + 0] = pv; a.prev[b * 2 + 1] = pw;
        a.root[b] = root; a.status[b] = status; a.status_step[b] = status_step; a.done[b] = done;
    }
}

template <int GEO, bool LDSWIN, bool NEXT_LDS, bool JUMP>
hipError_t launch_t(const SolveParams &p, const AstarDwaArgs &a, hipStream_t s)
{
    const int threads = astar_dwa_threads(a.nv, a.nw);
    const size_t lds = astar_dwa_lds_bytes(p, a.nv, a.nw, a.H, a.W, NEXT_LDS);
    hipError_t e = ensure_lds(astar_dwa_kernel<GEO, LDSWIN, NEXT_LDS, JUMP>, lds);
    if (e != hipSuccess) return e;
    astar_dwa_kernel<GEO, LDSWIN, NEXT_LDS, JUMP><<<dim3(p.B), dim3(threads), lds, s>>>(p, a);
    return hipGetLastError();
}

template <int GEO>
hipError_t launch_g(const SolveParams &p, const AstarDwaArgs &a, hipStream_t s)
{
    const bool win = p.WN > 0;
    if (a.hops)                                            // the jump walk reads the tables from global memory, next not at all
        return win ? launch_t<GEO, true, false, true>(p, a, s) : launch_t<GEO, false, false, true>(p, a, s);
    const bool nl = astar_dwa_lds_bytes(p, a.nv, a.nw, a.H, a.W, true) <= 160 * 1024;
    if (win) return nl ? launch_t<GEO, true, true, false>(p, a, s) : launch_t<GEO, true, false, false>(p, a, s);
    return nl ? launch_t<GEO, false, true, false>(p, a, s) : launch_t<GEO, false, false, false>(p, a, s);
}

}  // namespace

int astar_dwa_threads(int nv, int nw)
{
    return ((nv * nw + 63) / 64) * 64;
}

size_t astar_dwa_lds_bytes(const SolveParams &p, int nv, int nw, int H, int W, bool next_in_lds)
{
    const size_t floats = (size_t)p.WN * p.WN + 32 + 2 * (size_t)nv * nw + astar_dwa_threads(nv, nw) + 4;
    return floats * 4 + (next_in_lds ? (((size_t)H * W + 3) & ~(size_t)3) : 0);
}

hipError_t launch_astar_dwa(const SolveParams &p, const AstarDwaArgs &a, hipStream_t s)
{
    switch (geo_of(p)) {
    case kGeoPow2Origin0: return launch_g<kGeoPow2Origin0>(p, a, s);
    case kGeoPow2: return launch_g<kGeoPow2>(p, a, s);
    default: return launch_g<kGeoGeneral>(p, a, s);
    }
}

}  // namespace bn
