// astar_dwa.h -- launch interface of the fused A* + DWA episode (astar_dwa.hip) for the C ABI (mppi_loops.cpp).
#pragma once
#include "astar_view.h"
#include "episode_rows.h"
#include "mppi_kernels.h"

namespace bn {

constexpr int kAstarDwaStepsPerLaunch = 256;   // control steps per launch: bounds a kernel's duration, keeps a fault attributable to a chunk
constexpr int64_t kAstarDwaNodesPerLaunch = (int64_t)1 << 20;   // ... and at most this many map cells x steps (a step's walks are O(H W))

struct AstarDwaArgs {
    const uint8_t *next;          // (B, H, W) the A* handle's next-hop maps
    const float *arisk;           // (B, H, W) its risk maps (the goal's collision test, astar.py:93-94)
    const AStarInst *ainst;       // (B) its goal cells and stuck thresholds
    const int32_t *aerr;          // its field kernel's error word
    const int32_t *hops;          // (B, H, W) its jump tables (walk mode 1; nullptr: the serial walk): hops to the goal, -1 unreachable
    const int32_t *jump;          // (B, levels, H, W) the cell 2^k hops on
    const int32_t *jerr;          // the table build's error word
    int levels;
    int H, W;
    float *state;                 // (B, 3) in/out: the environment states
    float *prev;                  // (B, 2) in/out: the window centre (the previous argmin action, dwa.py:147)
    int32_t *root;                // (B) in/out: iy * W + ix of the last start cell whose walk reached the goal, or -1
    int32_t *status, *status_step, *done;   // (B) in/out: bn_astar_dwa_status, the step it was set at, first goal step or -1
    EpisodeRows log;              // this call's states, rewards and actions
    float *log_subgoal;           // (cap, B, 2) the stage-cost target of each step
    const float *z;               // (n, B) injected slip draws, or nullptr: Philox keyed by (env seed, step0 + step)
    int32_t *err;                 // device error word of the handle: bit 0 = a next-hop walk exceeded H*W nodes or hit an unreachable cell
    float alim0, alim1, dwa_dt, lookahead;
    int nv, nw;
    uint64_t step0;               // episode step (since bn_astar_dwa_reset) of the call's first step
    int s0, ns;                   // this launch runs the call's steps [s0, s0 + ns)
};

size_t astar_dwa_lds_bytes(const SolveParams &p, int nv, int nw, int H, int W, bool next_in_lds);
int astar_dwa_threads(int nv, int nw);
// grid = B, one workgroup per instance; the next-hop map is staged in LDS when it fits.  a.hops set: the lanes fetch the path's
// nodes through the jump tables instead of lane 0 walking next (which is then not read)
hipError_t launch_astar_dwa(const SolveParams &p, const AstarDwaArgs &a, hipStream_t s);

}  // namespace bn
