// astar_view.h -- what the fused A* + DWA episode (bn_astar_dwa_episode_async, astar_dwa.hip) reads of an A* handle: the device
// buffers of its latest solve and the event behind it.  Library-internal (astar_kernels.hip implements it); not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct bn_astar;

namespace bn {

struct AStarInst {           // == astar_kernels.hip's per-instance parameters, as the device holds them
    int32_t gx, gy;          // goal cell; gx < 0: the goal is out of bounds
    float thr;               // stuck threshold: collision = risk <= thr
    int32_t pad;
};

struct AStarView {
    int device, H, W, B;
    const uint8_t *next;      // (B, H, W): 0-7 a direction of astar.py:154-163, 8 the goal, 255 unreachable
    const float *risk;        // (B, H, W)
    const AStarInst *inst;    // (B)
    const int32_t *err;       // the field kernel's error word (non-zero: the solve failed)
    hipEvent_t solved;        // recorded behind the latest solve's kernels
};

// BN_ERR_STATE before the first bn_astar_solve_async
int astar_view(bn_astar *a, AStarView *v);
// Work enqueued on `s` reads the buffers above: the next bn_astar_set_map / bn_astar_solve_async / bn_astar_destroy waits for it.
int astar_add_reader(bn_astar *a, hipStream_t s);

}  // namespace bn
