// mppi_grid.h -- which workgroup of which instance a block of the rollout grid is, and the time steps per phase.
#pragma once
#include "mppi_kernels.h"

namespace bn {

namespace {

constexpr int TU = kChunk;   // time steps per phase (chunk): chain works on chunk c, consumers on c-1, producers on c+2

// Which workgroup of which instance this is (see rollout_grid): rollout workgroup `blk` of instance `b`, or the aux
// workgroup of instance `b` (tail of the previous solve).  Rows past the instances hold the aux workgroups, so they are
// dispatched last; with xs = 3 the workgroups of one instance share an XCD (and its L2: window rows, partials).
struct WgId { int b, blk; bool aux, idle, self; };   // self: the aux workgroup that writes the tail of THIS launch's solve (SolveParams::self_tail)

__device__ __forceinline__ WgId decode_wg(const SolveParams &p)
{
    const int rows = (p.B + (1 << p.xs) - 1) >> p.xs;
    WgId r;
    r.self = false;
    if ((int)blockIdx.y >= rows) {
        r.aux = true;
        r.blk = p.nblk;
        r.b = ((int)blockIdx.y - rows) * (int)gridDim.x + (int)blockIdx.x;
        if (p.self_tail && r.b >= (p.have_prev ? p.B : 0)) {            // behind the previous solve's tails: this solve's own
            r.self = true;
            r.b -= p.have_prev ? p.B : 0;
        }
    } else {
        r.aux = false;
        r.blk = (int)blockIdx.x >> p.xs;
        r.b = ((int)blockIdx.y << p.xs) + ((int)blockIdx.x & ((1 << p.xs) - 1));
    }
    r.idle = r.b >= p.B;
    return r;
}

}  // namespace

}  // namespace bn
