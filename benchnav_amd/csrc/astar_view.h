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
    // the jump tables (bn_astar_jump_build_async); jump_current: built behind the latest solve and not stale
    bool jump_current;
    int levels;               // kept levels, max(1, ceil(log2(H W)))
    const int32_t *hops;      // (B, H, W): hops to the goal, -1 unreachable
    const int32_t *jump;      // (B, levels, H, W): the cell 2^k hops on
    const int32_t *jerr;      // the build's error word (non-zero: next is not a valid next-hop map)
    hipEvent_t jump_built;    // recorded behind the latest build
};

// BN_ERR_STATE before the first bn_astar_solve_async
int astar_view(bn_astar *a, AStarView *v);
// Work enqueued on `s` reads the buffers above (the tables included): the next bn_astar_set_map / bn_astar_solve_async /
// bn_astar_jump_build_async / bn_astar_destroy waits for it.  The handle keeps one event for all readers: where the previous
// reader was enqueued on another stream, `s` is made to wait for it on the device (hipStreamWaitEvent; the host is not blocked)
// before the event is recorded again, so work enqueued on `s` after this call runs behind that earlier reader too.
int astar_add_reader(bn_astar *a, hipStream_t s);

}  // namespace bn
