// episode_rows.h -- the three columns every closed loop logs, as a kernel sees them: what the A* + DWA episode (astar_dwa.hip) and
// the CL-RRT follow kernel (clrrt_loop.hip) carry in their arguments and write a row of.  The host fills it from the log's
// descriptor (episode_log.h).  Device-visible, no host toolkit.
#pragma once
#include <hip/hip_runtime.h>

namespace bn {

struct EpisodeRows {
    float *states;                // (cap + 1, B, 3) row 0 = the call's start, row i + 1 = the state after row i of the call
    float *reward;                // (cap, B)
    float *action;                // (cap, B, 2)

    // row `row` of instance b (one lane; grid = B): returns the row's index row * B + b for the caller's own columns
    __device__ __forceinline__ size_t write(int row, int b, float x, float y, float th, float rw, float u0, float u1) const
    {
        const size_t B = gridDim.x, r = (size_t)row * B + b;
        float *ls = states + (r + B) * 3;
        ls[0] = x; ls[1] = y; ls[2] = th;
        reward[r] = rw;
        action[r * 2 + 0] = u0; action[r * 2 + 1] = u1;
        return r;
    }
};

}  // namespace bn
