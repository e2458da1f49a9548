// astar_kernels.hip -- the A* global planner as one goal-rooted shortest-path solve per (map, goal).
//
// Replaces AStar.forward (reference src/planners/global_planners/search_based/astar.py:73-122), a host best-first search run
// anew on every control step.  Every call searches toward the SAME goal on the SAME maps (the constructor fixes both,
// astar.py:55-71) and the edge weight is symmetric, so one cost-to-go field rooted at the goal serves every start:
//   D[goal] = 0,  D[n] = min over edges n->m of fl32(w(n,m) + D[m])            (n, m not in collision)
//   next[n] = first minimiser of fl32(w(n,m) + D[m]) in the reference's direction order (every cell, collision cells too)
// and AStar.forward becomes an O(path length) pointer walk over `next` on the host (bn_astar_path).
//
// Graph (astar.py): cells (ix, iy), arrays indexed [iy, ix] (_get_value :230-241); an edge a->b for each of the 8 neighbours b
// in bounds that is not a collision (_get_neighbors :142-167); collision = risk[iy, ix] <= stuck_threshold (_is_collision
// :182-192; NaN risk is traversable); weight (_distance :124-140, NumPy 2 scalar arithmetic)
//   w = sqrt_f32( f32(dx^2 + dy^2) + f32(dz * dz) ),  dx, dy = |d index| * resolution in double,  dz = |h_a - h_b| in f32.
//
// fl32(w + d) is monotone in d and w > 0, so fair relaxation in ANY order reaches the same fixpoint as a Dijkstra in the same
// arithmetic: the field is bit-exact and bit-identical run to run although workgroups race.
//
// Kernel: a persistent tile worklist.  Each map is cut into 32x32 tiles with one dirty flag each.  A workgroup claims a dirty
// tile (atomic exchange 1 -> 0), reads it and its 1-cell halo, relaxes it in LDS to its local fixpoint, publishes the improved
// cells with device-scope atomicMin (D >= 0, so the float order is the unsigned order), and re-flags every neighbouring tile
// whose halo holds an improved border cell.  `pending` counts dirty flags plus tiles in flight: the workers exit when it is 0.
// No co-residency is assumed (a workgroup that starts after the work is done exits at once), and every wait is bounded by
// a wall-clock deadline that reports through the error word.
// The host side takes its device guard and HIP check from bn_host.h.
#include "../../include/benchnav_mppi.h"
#include "bn_device_math.h"
#include "bn_host.h"
#include "astar_view.h"

#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace bn {
namespace {

constexpr int kTile = 32;                    // tile edge (cells)
constexpr int kHalo = kTile + 2;             // with the 1-cell halo
constexpr int kThreads = 256;                // 4 cells per thread: column tid % 32, rows tid / 32 + 8 k
constexpr int kCellsPerThread = kTile * kTile / kThreads;
constexpr int kMaxLocalIters = 4 * kHalo * kHalo;   // in-place relaxation of 1024 cells converges in <= 1024 sweeps
constexpr uint8_t kNextGoal = 8, kNextNone = 255;
// error word bits
constexpr int kErrDeadline = 1, kErrLocal = 2;

// the reference's direction order (astar.py:154-163), as (dx, dy) on (ix, iy)
__constant__ int8_t c_dx[8] = {-1, 1, 0, 0, -1, -1, 1, 1};
__constant__ int8_t c_dy[8] = {0, 0, -1, 1, -1, 1, -1, 1};
constexpr int8_t h_dx[8] = {-1, 1, 0, 0, -1, -1, 1, 1};
constexpr int8_t h_dy[8] = {0, 0, -1, 1, -1, 1, -1, 1};

using InstParams = AStarInst;   // goal cell (gx < 0: no goal, the field stays +inf everywhere), stuck threshold

struct FieldArgs {
    const float *heights;    // (B, H, W)
    const float *risk;       // (B, H, W)
    const InstParams *inst;  // (B)
    float *D;                // (B, H, W) cost-to-go, +inf where not reached
    uint8_t *next;           // (B, H, W)
    int32_t *flags;          // (B, TY, TX) dirty flags
    int32_t *ctl;            // [0] pending, [1] error word
    int H, W, B, TX, TY;
    float p_axis, p_diag;    // f32(res^2), f32(res^2 + res^2): the planar terms, rounded once from double
    uint64_t deadline_ticks; // wall-clock bound of the field kernel
};

__device__ __forceinline__ bool is_free(float r, float thr) { return !(r <= thr); }

__device__ __forceinline__ float edge_w(float p, float ha, float hb)
{
    const float dz = fabsf(ha - hb);
    return sqrt_cr(p + dz * dz);             // -ffp-contract=off: a rounded product, then a rounded sum
}

__device__ __forceinline__ uint32_t atomic_read_u32(uint32_t *p)
{
    return __hip_atomic_fetch_or(p, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // served where the atomics are
}
__device__ __forceinline__ int32_t atomic_read_i32(int32_t *p)
{
    return __hip_atomic_fetch_or(p, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// D = +inf, D[goal] = 0 where the goal is in bounds and free, and every tile whose halo holds the goal flagged: its own tile
// and, for a goal on a tile border, the neighbouring tiles across it.  The field kernel never publishes the goal (its value
// starts at 0 and cannot fall), so a goal whose only free neighbours lie in another tile is seen there through this flag alone.
__global__ __launch_bounds__(256) void astar_init_kernel(FieldArgs a)
{
    const size_t cells = (size_t)a.H * a.W;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cells * a.B) return;
    const int b = (int)(i / cells);
    const int c = (int)(i - (size_t)b * cells);
    const int ix = c % a.W, iy = c / a.W;
    const InstParams p = a.inst[b];
    const bool goal = p.gx == ix && p.gy == iy && is_free(a.risk[i], p.thr);
    a.D[i] = goal ? 0.0f : INFINITY;
    if (goal) {
        const int tx = ix / kTile, ty = iy / kTile, cx = ix % kTile, cy = iy % kTile;
        const int x_lo = cx == 0 ? -1 : 0, x_hi = cx == kTile - 1 ? 1 : 0;
        const int y_lo = cy == 0 ? -1 : 0, y_hi = cy == kTile - 1 ? 1 : 0;
        for (int ey = y_lo; ey <= y_hi; ++ey)
            for (int ex = x_lo; ex <= x_hi; ++ex) {
                const int ntx = tx + ex, nty = ty + ey;
                if (ntx < 0 || ntx >= a.TX || nty < 0 || nty >= a.TY) continue;
                a.flags[(size_t)b * a.TX * a.TY + nty * a.TX + ntx] = 1;
                atomicAdd(&a.ctl[0], 1);
            }
    }
}

__global__ __launch_bounds__(kThreads) void astar_field_kernel(FieldArgs a)
{
    __shared__ float s_D[kHalo * kHalo];
    __shared__ float s_h[kHalo * kHalo];
    __shared__ uint8_t s_free[kHalo * kHalo];
    __shared__ int s_pick, s_cmd, s_mask;

    const int tid = threadIdx.x;
    const int NT = a.B * a.TX * a.TY;
    const int tiles_per_inst = a.TX * a.TY;
    const uint64_t t0 = wall_clock64();
    int window = (int)(((uint64_t)blockIdx.x * kThreads) % (uint64_t)NT);
    const int scan = NT < kThreads ? NT : kThreads;

    for (;;) {
        // ---- find and claim one dirty tile ------------------------------------------------------------------------------
        if (tid == 0) s_pick = 0x7fffffff;
        __syncthreads();
        if (tid < scan) {
            int t = window + tid;
            if (t >= NT) t -= NT;
            if (atomic_read_i32(&a.flags[t])) atomicMin(&s_pick, t);
        }
        __syncthreads();
        if (tid == 0) {
            int cmd = -1;                                  // -1: nothing claimed, -2: exit
            if (s_pick != 0x7fffffff &&
                __hip_atomic_exchange(&a.flags[s_pick], 0, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == 1) {
                cmd = s_pick;
            } else {
                if (atomic_read_i32(&a.ctl[0]) == 0 || atomic_read_i32(&a.ctl[1]) != 0) cmd = -2;
                else if (wall_clock64() - t0 > a.deadline_ticks) {
                    atomicOr(&a.ctl[1], kErrDeadline);
                    cmd = -2;
                }
            }
            s_cmd = cmd;
            s_mask = 0;
        }
        __syncthreads();
        const int tile = s_cmd;
        if (tile == -2) return;
        if (tile == -1) {
            window += scan;
            if (window >= NT) window -= NT;
            __builtin_amdgcn_s_sleep(8);
            continue;
        }

        // ---- load the tile and its halo -------------------------------------------------------------------------------
        const int b = tile / tiles_per_inst;
        const int tr = tile - b * tiles_per_inst;
        const int ty = tr / a.TX, tx = tr - ty * a.TX;
        const int x0 = tx * kTile - 1, y0 = ty * kTile - 1;       // global cell of halo (0, 0)
        const size_t base = (size_t)b * a.H * a.W;
        const float thr = a.inst[b].thr;
        for (int j = tid; j < kHalo * kHalo; j += kThreads) {
            const int hx = j % kHalo, hy = j / kHalo;
            const int gx = x0 + hx, gy = y0 + hy;
            float d = INFINITY, h = 0.0f;
            uint8_t f = 0;
            if (gx >= 0 && gx < a.W && gy >= 0 && gy < a.H) {
                const size_t g = base + (size_t)gy * a.W + gx;
                h = a.heights[g];
                f = is_free(a.risk[g], thr) ? 1 : 0;
                if (f) d = __uint_as_float(atomic_read_u32(reinterpret_cast<uint32_t *>(a.D + g)));
            }
            s_D[j] = d; s_h[j] = h; s_free[j] = f;
        }
        __syncthreads();

        // per-cell edge weights, +inf to a neighbour that is out of bounds or in collision
        const int cx = tid % kTile;
        float w[kCellsPerThread][8];
        float d0[kCellsPerThread];
        bool active[kCellsPerThread];
#pragma unroll
        for (int k = 0; k < kCellsPerThread; ++k) {
            const int cy = tid / kTile + 8 * k;
            const int hj = (cy + 1) * kHalo + cx + 1;
            active[k] = s_free[hj] != 0;            // a collision cell has no incoming edge: it never gets a value
            d0[k] = s_D[hj];
            const float hc = s_h[hj];
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                const int nj = hj + c_dy[d] * kHalo + c_dx[d];
                w[k][d] = s_free[nj] ? edge_w(d < 4 ? a.p_axis : a.p_diag, hc, s_h[nj]) : INFINITY;
            }
        }

        // ---- relax to the tile's local fixpoint (in place: values only fall, each one a realised path cost) -----------
        int iters = 0;
        for (;;) {
            int changed = 0;
#pragma unroll
            for (int k = 0; k < kCellsPerThread; ++k) {
                if (!active[k]) continue;
                const int hj = (tid / kTile + 8 * k + 1) * kHalo + cx + 1;
                float best = s_D[hj];
#pragma unroll
                for (int d = 0; d < 8; ++d) {
                    const float cand = w[k][d] + s_D[hj + c_dy[d] * kHalo + c_dx[d]];
                    if (cand < best) best = cand;
                }
                if (best < s_D[hj]) { s_D[hj] = best; changed = 1; }
            }
            if (!__syncthreads_or(changed)) break;
            if (++iters > kMaxLocalIters) {
                if (tid == 0) atomicOr(&a.ctl[1], kErrLocal);
                break;
            }
        }

        // ---- publish improved cells; collect the neighbouring tiles whose halo changed ----------------------------------
        int mask = 0;
#pragma unroll
        for (int k = 0; k < kCellsPerThread; ++k) {
            const int cy = tid / kTile + 8 * k;
            const int hj = (cy + 1) * kHalo + cx + 1;
            const float v = s_D[hj];
            const int gx = x0 + 1 + cx, gy = y0 + 1 + cy;
            if (!active[k] || !(v < d0[k]) || gx >= a.W || gy >= a.H) continue;
            const uint32_t vb = __float_as_uint(v);
            const uint32_t old = __hip_atomic_fetch_min(reinterpret_cast<uint32_t *>(a.D + base + (size_t)gy * a.W + gx), vb,
                                                        __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (vb < old) {
                const int ex = cx == 0 ? -1 : (cx == kTile - 1 ? 1 : 0);
                const int ey = cy == 0 ? -1 : (cy == kTile - 1 ? 1 : 0);
                if (ex) mask |= 1 << ((0 + 1) * 3 + ex + 1);
                if (ey) mask |= 1 << ((ey + 1) * 3 + 0 + 1);
                if (ex && ey) mask |= 1 << ((ey + 1) * 3 + ex + 1);
            }
        }
        if (mask) atomicOr(&s_mask, mask);
        __syncthreads();
        if (tid == 0) {
            // every published atomicMin above has returned; the release orders them before the flags
            const int m = s_mask;
            for (int e = 0; e < 9; ++e) {
                if (!(m >> e & 1)) continue;
                const int ntx = tx + e % 3 - 1, nty = ty + e / 3 - 1;
                if (ntx < 0 || ntx >= a.TX || nty < 0 || nty >= a.TY) continue;
                const int nt = b * tiles_per_inst + nty * a.TX + ntx;
                if (__hip_atomic_exchange(&a.flags[nt], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == 0)
                    __hip_atomic_fetch_add(&a.ctl[0], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            }
            __hip_atomic_fetch_add(&a.ctl[0], -1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);   // this tile is done
        }
        __syncthreads();
    }
}

// next[n]: first minimiser of fl32(w(n, m) + D[m]) over the 8 neighbours in direction order; D is +inf on collision cells,
// so they are never chosen.  kNextGoal at the goal, kNextNone where no candidate is finite.
__global__ __launch_bounds__(256) void astar_next_kernel(FieldArgs a)
{
    const size_t cells = (size_t)a.H * a.W;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cells * a.B) return;
    const int b = (int)(i / cells);
    const int c = (int)(i - (size_t)b * cells);
    const int ix = c % a.W, iy = c / a.W;
    const InstParams p = a.inst[b];
    if (p.gx == ix && p.gy == iy && a.D[i] == 0.0f) { a.next[i] = kNextGoal; return; }
    const float hc = a.heights[i];
    float best = INFINITY;
    uint8_t arg = kNextNone;
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        const int nx = ix + c_dx[d], ny = iy + c_dy[d];
        if (nx < 0 || nx >= a.W || ny < 0 || ny >= a.H) continue;
        const size_t j = (size_t)b * cells + (size_t)ny * a.W + nx;
        const float cand = edge_w(d < 4 ? a.p_axis : a.p_diag, hc, a.heights[j]) + a.D[j];
        if (cand < best) { best = cand; arg = (uint8_t)d; }
    }
    a.next[i] = arg;
}

// ---- jump tables: pointer doubling over next ------------------------------------------------------------------------------
// jump[k][c] = the cell 2^k hops from c along next (the goal and cells without a hop map to themselves); hops[c] = hops from c
// to the goal, -1 where the walk ends on kNextNone.  Cell indices (iy * W + ix) are int32 at every map size.  levels =
// max(1, ceil(log2(H W))) levels are kept whatever the largest hop count is: a path has at most H W nodes, so every node index
// is a sum of kept powers of two.  Footprint: B * (levels + 2) * H W * 4 bytes (the levels and two hop buffers, read and
// written in turn), e.g. 64^2: 224 KiB * B, 256^2: 4.5 MiB * B, 512^2: 20 MiB * B.
//
// The build is levels + 1 launches in stream order (level 0, levels - 1 doublings, one closing round), a fixed number whatever
// the map holds, one thread per cell, every index read from a table written by an earlier launch and in bounds by construction:
// a corrupt map can neither hang nor misdirect it.  Validation: level 0 rejects a code in 9-254 and a hop off the map (the cell
// then maps to itself); the closing round composes level levels - 1 with itself, 2^levels >= H W hops, and a cell that is then
// still on a stepping cell lies on, or leads into, a cycle.  Each sets a bit of the tables' error word and the smallest
// offending cell index next to it.
struct JumpArgs {
    const uint8_t *next;     // (B, H, W)
    int32_t *jump;           // (B, levels, H W)
    const int32_t *hops_in;  // (B, H W) hops within the 2^k already composed
    int32_t *hops_out;
    int32_t *err;            // [0] error bits, [1] smallest offending cell (b * H W + c)
    int H, W, B, levels, k;
};
constexpr int kJumpBadCode = 1, kJumpOffMap = 2, kJumpCycle = 4;

__device__ __forceinline__ void jump_report(int32_t *err, int bit, size_t i)
{
    atomicOr(&err[0], bit);
    atomicMin(&err[1], (int32_t)i);
}

__global__ __launch_bounds__(256) void astar_jump_init_kernel(JumpArgs a)
{
    const size_t cells = (size_t)a.H * a.W;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cells * a.B) return;
    const int b = (int)(i / cells);
    const int c = (int)(i - (size_t)b * cells);
    const uint32_t code = a.next[i];
    int tgt = c, hp = 0;
    if (code < kNextGoal) {
        const int nx = c % a.W + c_dx[code], ny = c / a.W + c_dy[code];
        if (nx < 0 || nx >= a.W || ny < 0 || ny >= a.H) jump_report(a.err, kJumpOffMap, i);
        else { tgt = ny * a.W + nx; hp = 1; }
    } else if (code != kNextGoal && code != kNextNone) {
        jump_report(a.err, kJumpBadCode, i);
    }
    a.jump[(size_t)b * a.levels * cells + c] = tgt;
    a.hops_out[i] = hp;
}

// level k -> k + 1
__global__ __launch_bounds__(256) void astar_jump_level_kernel(JumpArgs a)
{
    const size_t cells = (size_t)a.H * a.W;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cells * a.B) return;
    const int b = (int)(i / cells);
    const int c = (int)(i - (size_t)b * cells);
    int32_t *lv = a.jump + ((size_t)b * a.levels + a.k) * cells;
    const int j = lv[c];
    lv[cells + c] = lv[j];
    a.hops_out[i] = a.hops_in[i] + a.hops_in[(size_t)b * cells + j];
}

// the closing round: 2^levels hops from every cell, the final hop counts and the cycle test
__global__ __launch_bounds__(256) void astar_jump_close_kernel(JumpArgs a)
{
    const size_t cells = (size_t)a.H * a.W;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cells * a.B) return;
    const int b = (int)(i / cells);
    const int c = (int)(i - (size_t)b * cells);
    const int32_t *lv = a.jump + ((size_t)b * a.levels + a.levels - 1) * cells;
    const int j = lv[c];
    const int e = lv[j];
    int hp = a.hops_in[i] + a.hops_in[(size_t)b * cells + j];
    const uint32_t code = a.next[(size_t)b * cells + e];
    if (code < kNextGoal) { jump_report(a.err, kJumpCycle, i); hp = -1; }
    else if (code != kNextGoal) hp = -1;
    a.hops_out[i] = hp;
}

// One thread per (start, node index): node k of the path from a start is the start advanced over the set bits of k.
struct PathsArgs {
    const int32_t *hops;     // (H W) of the instance
    const int32_t *jump;     // (levels, H W) of the instance
    const int32_t *starts;   // (n, 2) (ix, iy)
    int32_t *out_xy;         // (n, max_len, 2)
    int32_t *out_len;        // (n)
    int H, W, n, max_len;
};

__global__ __launch_bounds__(256) void astar_paths_kernel(PathsArgs a)
{
    const int row = a.max_len > 0 ? a.max_len : 1;
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (size_t)a.n * row) return;
    const int i = (int)(id / row);
    const int k = (int)(id - (size_t)i * row);
    const int sx = a.starts[2 * i], sy = a.starts[2 * i + 1];
    const size_t cells = (size_t)a.H * a.W;
    int len = -1, x = -1, y = -1;
    if (sx >= 0 && sx < a.W && sy >= 0 && sy < a.H) {
        int c = sy * a.W + sx;
        len = a.hops[c] + 1;                     // -1 hops: unreachable, 0 nodes
        if (k < len) {                           // k <= hops < H W <= 2^levels: every set bit is a kept level
            for (int r = k, lvl = 0; r; r >>= 1, ++lvl)
                if (r & 1) c = a.jump[lvl * cells + c];
            x = c % a.W; y = c / a.W;
        }
    }
    if (k == 0) a.out_len[i] = len;
    if (k < a.max_len) {
        a.out_xy[2 * id] = x;
        a.out_xy[2 * id + 1] = y;
    }
}

thread_local std::string g_astar_error;

}  // namespace
}  // namespace bn

struct bn_astar {
    int device = 0, H = 0, W = 0, B = 0, TX = 0, TY = 0;
    double resolution = -1.0;                  // planar terms are set with the first map
    float p_axis = 0.0f, p_diag = 0.0f;
    float *heights = nullptr, *risk = nullptr, *D = nullptr;
    uint8_t *next = nullptr;
    int32_t *flags = nullptr, *ctl = nullptr;
    bn::InstParams *inst_dev = nullptr;
    std::vector<bn::InstParams> inst;           // host mirror, uploaded by every solve
    std::vector<uint8_t> have_map;
    bn::InstParams *inst_pinned = nullptr;
    uint8_t *next_host = nullptr;               // pinned copy of `next`, refreshed by every solve
    int32_t *ctl_host = nullptr;
    hipEvent_t ev_start = nullptr, ev_kernels = nullptr, ev_done = nullptr;
    hipEvent_t ev_reader = nullptr;             // behind the latest fused episode that reads the buffers (bn::astar_add_reader)
    bool solved = false, pending_check = false, reader_pending = false;
    hipStream_t reader_stream = nullptr;        // the stream ev_reader was last recorded on
    uint64_t deadline_ticks = 0;
    // jump tables (bn_astar_jump_build_async), allocated by the first build
    int levels = 1;
    int32_t *jump = nullptr;                    // (B, levels, H W)
    int32_t *hopbuf[2] = {nullptr, nullptr};    // (B, H W) each; the closing round writes hopbuf[0]
    int32_t *jerr = nullptr, *jerr_host = nullptr;   // error bits, smallest offending cell; the pinned copy of the latest build
    int32_t *starts_dev = nullptr;              // staging of host-side starts (bn_astar_paths_async)
    size_t starts_cap = 0;
    hipEvent_t ev_jump_start = nullptr, ev_jump_kernels = nullptr, ev_jump_done = nullptr;
    bool jump_valid = false, jump_pending = false;   // built behind the latest solve and not stale; error word not yet read
    bn::DeviceBuffers bufs, jumps;              // the table of all of the above (bn_host.h); `jumps` is built by the first table build
};

namespace {

int astar_fail(int code, const std::string &msg)
{
    bn::g_astar_error = msg;
    return code;
}

#define ASTAR_HIP(expr) BN_HIP_AS(astar_fail, expr, #expr)
#define ASTAR_ON_DEVICE(h) BN_ON_DEVICE(astar_fail, (h)->device)

// an enqueued episode still reads the buffers: wait for it before they are rewritten or freed
void wait_readers(bn_astar_t *h)
{
    if (h->jump_pending) {                       // a table build still reads next
        (void)hipEventSynchronize(h->ev_jump_done);
        h->jump_pending = false;
    }
    if (!h->reader_pending) return;
    (void)hipEventSynchronize(h->ev_reader);
    h->reader_pending = false;
}

// BN_OK when the tables are current and their build found next valid (waits for a pending build)
int jump_ready(bn_astar_t *h)
{
    if (!h->jump_valid)
        return astar_fail(BN_ERR_STATE, "the jump tables are stale or were never built: bn_astar_jump_build_async must follow the latest "
                                        "bn_astar_set_map / bn_astar_set_goal / bn_astar_solve_async");
    if (h->jump_pending) {
        ASTAR_HIP(hipEventSynchronize(h->ev_jump_done));
        h->jump_pending = false;
    }
    const int bits = h->jerr_host[0];
    if (bits != 0) {
        const int64_t cells = (int64_t)h->H * h->W, i = (uint32_t)h->jerr_host[1];
        const int64_t c = i % cells;
        return astar_fail(BN_ERR_STATE, std::string("jump tables: next is not a valid next-hop map (") +
                                        ((bits & bn::kJumpBadCode) ? "unknown code; " : "") + ((bits & bn::kJumpOffMap) ? "hop off the map; " : "") +
                                        ((bits & bn::kJumpCycle) ? "cycle; " : "") + "first at instance " + std::to_string(i / cells) +
                                        ", cell (" + std::to_string(c % h->W) + ", " + std::to_string(c / h->W) + "))");
    }
    return BN_OK;
}

// waits for the last solve, copies nothing: the pinned `next` and error word are already on the host
int astar_wait(bn_astar_t *h)
{
    if (!h->solved) return astar_fail(BN_ERR_STATE, "no solve has been enqueued");
    if (h->pending_check) {
        ASTAR_HIP(hipEventSynchronize(h->ev_done));
        h->pending_check = false;
    }
    if (h->ctl_host[1] != 0)
        return astar_fail(BN_ERR_STATE, std::string("field solve failed: ") +
                                        ((h->ctl_host[1] & bn::kErrDeadline) ? "deadline exceeded " : "") +
                                        ((h->ctl_host[1] & bn::kErrLocal) ? "tile relaxation did not converge" : ""));
    return BN_OK;
}

// What bn_astar_create builds: every buffer, pinned block and event of the handle entered in its tables, the solve's allocated.
int astar_init(bn_astar_t *h)
{
    const int B = h->B;
    const size_t cells = (size_t)h->H * h->W * B;
    h->inst.assign(B, bn::InstParams{-1, -1, 0.0f, 0});
    h->have_map.assign(B, 0);
    bn::DeviceBuffers &m = h->bufs, &j = h->jumps;
    m.add(&h->heights, cells * 4); m.add(&h->risk, cells * 4); m.add(&h->D, cells * 4); m.add(&h->next, cells);
    m.add(&h->flags, (size_t)B * h->TX * h->TY * 4); m.add(&h->ctl, 4 * 4); m.add(&h->inst_dev, sizeof(bn::InstParams) * B);
    m.add_later(&h->starts_dev);                // grows with the largest n of host starts (starts_cap)
    m.add_pinned(&h->inst_pinned, sizeof(bn::InstParams) * B); m.add_pinned(&h->next_host, cells); m.add_pinned(&h->ctl_host, 4 * 4);
    m.add_event(&h->ev_start); m.add_event(&h->ev_kernels); m.add_event(&h->ev_done);
    m.add_event(&h->ev_reader, hipEventDisableTiming);
    j.add(&h->hopbuf[0], cells * 4); j.add(&h->hopbuf[1], cells * 4); j.add(&h->jerr, 2 * 4); j.add_pinned(&h->jerr_host, 2 * 4);
    j.add_event(&h->ev_jump_start); j.add_event(&h->ev_jump_kernels); j.add_event(&h->ev_jump_done);
    j.add(&h->jump, cells * h->levels * 4);
    if (int rc = m.alloc_all(astar_fail)) return rc;
    int clock_khz = 0;
    ASTAR_HIP(hipDeviceGetAttribute(&clock_khz, hipDeviceAttributeWallClockRate, h->device));
    std::memset(h->ctl_host, 0, 16);
    h->deadline_ticks = (uint64_t)(clock_khz > 0 ? clock_khz : 100000) * 1000ull * 5ull;    // 5 s
    return BN_OK;
}

}  // namespace

extern "C" {

const char *bn_astar_last_error(void) { return bn::g_astar_error.c_str(); }

/* astar.py:33-71 (the constructor's buffers): B instances of one H x W shape on `device_id`. */
int bn_astar_create(int32_t device_id, int32_t H, int32_t W, int32_t B, bn_astar_t **out)
{
    if (!out) return astar_fail(BN_ERR_INVALID, "null handle pointer");
    *out = nullptr;
    if (H < 1 || W < 1 || B < 1 || (int64_t)H * W > (1 << 26) || (int64_t)H * W * B > ((int64_t)1 << 31))
        return astar_fail(BN_ERR_INVALID, "H, W, B must be >= 1 and the field must fit 2^31 cells");
    if (int rc = bn::open_device(device_id, astar_fail)) return rc;
    BN_ON_DEVICE(astar_fail, device_id);
    auto *h = new bn_astar_t();
    h->device = device_id; h->H = H; h->W = W; h->B = B;
    h->TX = (W + bn::kTile - 1) / bn::kTile;
    h->TY = (H + bn::kTile - 1) / bn::kTile;
    while (((int64_t)1 << h->levels) < (int64_t)H * W) ++h->levels;
    if (int rc = astar_init(h)) {
        bn_astar_destroy(h);                    // leaves the error text as astar_init set it
        return rc;
    }
    *out = h;
    return BN_OK;
}

void bn_astar_destroy(bn_astar_t *h)
{
    if (!h) return;
    bn::DeviceGuard guard(h->device);
    if (h->pending_check) (void)hipEventSynchronize(h->ev_done);
    wait_readers(h);
    h->jumps.free_all();
    h->bufs.free_all();
    delete h;
}

/* astar.py:53-58: heights = grid_map.tensors["heights"], travs = _traversability_model._risks, _stuck_threshold, resolution.
 * Both maps are (H, W) row-major, indexed [iy, ix]; `where` says where they live.  Device-resident maps are copied after a
 * device synchronisation (the producer's stream is finished first).  Every instance must use the same resolution. */
int bn_astar_set_map(bn_astar_t *h, int32_t inst, const float *heights, const float *risks, bn_mem_kind where,
                     float stuck_threshold, double resolution)
{
    if (!h || !heights || !risks) return astar_fail(BN_ERR_INVALID, "null argument");
    if (inst < 0 || inst >= h->B) return astar_fail(BN_ERR_INVALID, "instance out of range");
    if (!(resolution > 0.0) || !std::isfinite(resolution)) return astar_fail(BN_ERR_INVALID, "resolution must be finite and > 0");
    if (h->resolution > 0.0 && resolution != h->resolution) return astar_fail(BN_ERR_INVALID, "every instance must share one resolution");
    if (where != BN_MEM_HOST && where != BN_MEM_DEVICE) return astar_fail(BN_ERR_INVALID, "unknown memory kind");
    ASTAR_ON_DEVICE(h);
    if (h->pending_check) { ASTAR_HIP(hipEventSynchronize(h->ev_done)); h->pending_check = false; }
    wait_readers(h);
    const size_t cells = (size_t)h->H * h->W, off = cells * inst;
    if (where == BN_MEM_DEVICE) ASTAR_HIP(hipDeviceSynchronize());
    const hipMemcpyKind kind = where == BN_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    ASTAR_HIP(hipMemcpy(h->heights + off, heights, cells * 4, kind));
    ASTAR_HIP(hipMemcpy(h->risk + off, risks, cells * 4, kind));
    // _distance (:134-140): dx = |di| * resolution and dy likewise are Python floats, dx**2 + dy**2 a double, rounded to f32 once
    // when the f32 dz**2 is added
    h->resolution = resolution;
    h->p_axis = (float)(resolution * resolution + 0.0);
    h->p_diag = (float)(resolution * resolution + resolution * resolution);
    h->inst[inst].thr = stuck_threshold;
    h->have_map[inst] = 1;
    h->jump_valid = false;
    return BN_OK;
}

/* astar.py:71 (_goal_node = _pos_to_index(goal_pos)): the goal cell of instance `inst`.  An out-of-bounds or collision goal is
 * accepted (the reference raises only in forward(), :88-94): its field is +inf everywhere and every path is "none". */
int bn_astar_set_goal(bn_astar_t *h, int32_t inst, int32_t ix, int32_t iy)
{
    if (!h) return astar_fail(BN_ERR_INVALID, "null handle");
    if (inst < 0 || inst >= h->B) return astar_fail(BN_ERR_INVALID, "instance out of range");
    const bool in = ix >= 0 && ix < h->W && iy >= 0 && iy < h->H;
    h->inst[inst].gx = in ? ix : -1;
    h->inst[inst].gy = in ? iy : -1;
    h->jump_valid = false;
    return BN_OK;
}

/* astar.py:96-122 (the search), done once per (map, goal) for all B instances: the cost-to-go field D and the next-hop map,
 * then an async copy of `next` to pinned host memory.  Enqueued on `stream`; bn_astar_path / bn_astar_sync wait for it. */
int bn_astar_solve_async(bn_astar_t *h, void *stream)
{
    if (!h) return astar_fail(BN_ERR_INVALID, "null handle");
    for (int b = 0; b < h->B; ++b)
        if (!h->have_map[b]) return astar_fail(BN_ERR_STATE, "instance " + std::to_string(b) + " has no map");
    ASTAR_ON_DEVICE(h);
    if (h->pending_check) { ASTAR_HIP(hipEventSynchronize(h->ev_done)); h->pending_check = false; }   // pinned buffers are reused
    wait_readers(h);
    hipStream_t s = (hipStream_t)stream;
    const size_t cells = (size_t)h->H * h->W * h->B;
    const int NT = h->B * h->TX * h->TY;
    std::memcpy(h->inst_pinned, h->inst.data(), sizeof(bn::InstParams) * h->B);
    bn::FieldArgs a{h->heights, h->risk, h->inst_dev, h->D, h->next, h->flags, h->ctl,
                    h->H, h->W, h->B, h->TX, h->TY, h->p_axis, h->p_diag, h->deadline_ticks};
    ASTAR_HIP(hipEventRecord(h->ev_start, s));
    ASTAR_HIP(hipMemcpyAsync(h->inst_dev, h->inst_pinned, sizeof(bn::InstParams) * h->B, hipMemcpyHostToDevice, s));
    ASTAR_HIP(hipMemsetAsync(h->flags, 0, (size_t)NT * 4, s));
    ASTAR_HIP(hipMemsetAsync(h->ctl, 0, 16, s));
    const int blocks = (int)((cells + 255) / 256);
    bn::astar_init_kernel<<<blocks, 256, 0, s>>>(a);
    ASTAR_HIP(hipGetLastError());
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device);
    const int workers = NT < cus ? NT : cus;          // residency is not required; more workers than tiles would only scan
    bn::astar_field_kernel<<<workers, bn::kThreads, 0, s>>>(a);
    ASTAR_HIP(hipGetLastError());
    bn::astar_next_kernel<<<blocks, 256, 0, s>>>(a);
    ASTAR_HIP(hipGetLastError());
    ASTAR_HIP(hipEventRecord(h->ev_kernels, s));
    ASTAR_HIP(hipMemcpyAsync(h->next_host, h->next, cells, hipMemcpyDeviceToHost, s));
    ASTAR_HIP(hipMemcpyAsync(h->ctl_host, h->ctl, 16, hipMemcpyDeviceToHost, s));
    ASTAR_HIP(hipEventRecord(h->ev_done, s));
    h->solved = true;
    h->pending_check = true;
    h->jump_valid = false;
    return BN_OK;
}

/* Waits for the last solve and reports a kernel-side failure (the field kernel's bounded waits). */
int bn_astar_sync(bn_astar_t *h)
{
    if (!h) return astar_fail(BN_ERR_INVALID, "null handle");
    ASTAR_ON_DEVICE(h);
    int rc = astar_wait(h);
    if (rc != BN_OK || !h->jump_valid) return rc;
    return jump_ready(h);
}

/* Device time of the last solve's kernels (init, field, next), in ms: for the rate tool. */
int bn_astar_kernel_ms(bn_astar_t *h, float *ms)
{
    if (!h || !ms) return astar_fail(BN_ERR_INVALID, "null argument");
    ASTAR_ON_DEVICE(h);
    int rc = astar_wait(h);
    if (rc != BN_OK) return rc;
    ASTAR_HIP(hipEventElapsedTime(ms, h->ev_start, h->ev_kernels));
    return BN_OK;
}

/* astar.py:73-122 + _reconstruct_path :194-213 for the start cell (ix, iy): walks `next` on the host from the start to the
 * goal and writes the nodes (ix, iy) start first into out_xy (2 * max_len int32).  Returns the node count (the full count,
 * even where it exceeds max_len: only max_len nodes are written), 0 where the goal is unreachable (the reference's None),
 * BN_ERR_INVALID for a start out of bounds. */
int bn_astar_path(bn_astar_t *h, int32_t inst, int32_t ix, int32_t iy, int32_t *out_xy, int32_t max_len)
{
    if (!h) return astar_fail(BN_ERR_INVALID, "null handle");
    if (inst < 0 || inst >= h->B) return astar_fail(BN_ERR_INVALID, "instance out of range");
    if (ix < 0 || ix >= h->W || iy < 0 || iy >= h->H) return astar_fail(BN_ERR_INVALID, "start out of bounds");
    if (max_len > 0 && !out_xy) return astar_fail(BN_ERR_INVALID, "null output");
    ASTAR_ON_DEVICE(h);
    int rc = astar_wait(h);
    if (rc != BN_OK) return rc;
    const uint8_t *nx = h->next_host + (size_t)h->H * h->W * inst;
    const int64_t bound = (int64_t)h->H * h->W;       // D strictly falls along next: no node repeats
    int32_t n = 0;
    for (int64_t step = 0; step < bound; ++step) {
        if (n < max_len) { out_xy[2 * n] = ix; out_xy[2 * n + 1] = iy; }
        ++n;
        const uint8_t c = nx[(size_t)iy * h->W + ix];
        if (c == bn::kNextGoal) return n;
        if (c >= 8) return 0;
        ix += bn::h_dx[c];
        iy += bn::h_dy[c];
    }
    return astar_fail(BN_ERR_STATE, "next-hop walk exceeded H*W nodes");
}

/* Test hook: the device buffers of instance `inst` -- D (H*W float32) and next (H*W uint8: 0-7 a direction of astar.py:154-163,
 * 8 the goal, 255 unreachable).  Valid after bn_astar_sync. */
int bn_astar_buffers(bn_astar_t *h, int32_t inst, void **D_dev, void **next_dev)
{
    if (!h || !D_dev || !next_dev) return astar_fail(BN_ERR_INVALID, "null argument");
    if (inst < 0 || inst >= h->B) return astar_fail(BN_ERR_INVALID, "instance out of range");
    const size_t off = (size_t)h->H * h->W * inst;
    *D_dev = h->D + off;
    *next_dev = h->next + off;
    return BN_OK;
}

/* The jump tables behind the latest solve, for all B instances: levels + 1 launches on `stream`, ordered behind the solve's
 * kernels by an event, then an async copy of the error word to pinned memory (read by bn_astar_sync and the consumers). */
int bn_astar_jump_build_async(bn_astar_t *h, void *stream)
{
    if (!h) return astar_fail(BN_ERR_INVALID, "null handle");
    if (!h->solved) return astar_fail(BN_ERR_STATE, "no solve has been enqueued: bn_astar_solve_async must precede the table build");
    ASTAR_ON_DEVICE(h);
    wait_readers(h);                              // an earlier build (its pinned word), episodes and paths reading the old tables
    const size_t cells = (size_t)h->H * h->W, total = cells * h->B;
    h->jump_valid = false;                        // until this build is enqueued whole: a failure below leaves no current tables
    if (int rc = h->jumps.ensure(astar_fail)) return rc;      // all or nothing: after a failure the next build allocates again
    hipStream_t s = (hipStream_t)stream;
    ASTAR_HIP(hipStreamWaitEvent(s, h->ev_kernels, 0));
    ASTAR_HIP(hipEventRecord(h->ev_jump_start, s));
    ASTAR_HIP(hipMemsetAsync(h->jerr, 0, 4, s));
    ASTAR_HIP(hipMemsetAsync(h->jerr + 1, 0x7f, 4, s));            // above every cell index: atomicMin keeps the smallest
    const int blocks = (int)((total + 255) / 256);
    int w = h->levels & 1;                        // levels + 1 rounds write the hop buffers in turn; the last one writes hopbuf[0]
    bn::JumpArgs a{h->next, h->jump, nullptr, h->hopbuf[w], h->jerr, h->H, h->W, h->B, h->levels, 0};
    bn::astar_jump_init_kernel<<<blocks, 256, 0, s>>>(a);
    ASTAR_HIP(hipGetLastError());
    for (int k = 0; k + 1 < h->levels; ++k) {
        a.k = k; a.hops_in = h->hopbuf[w]; a.hops_out = h->hopbuf[w ^ 1]; w ^= 1;
        bn::astar_jump_level_kernel<<<blocks, 256, 0, s>>>(a);
        ASTAR_HIP(hipGetLastError());
    }
    a.hops_in = h->hopbuf[w]; a.hops_out = h->hopbuf[w ^ 1];
    bn::astar_jump_close_kernel<<<blocks, 256, 0, s>>>(a);
    ASTAR_HIP(hipGetLastError());
    ASTAR_HIP(hipEventRecord(h->ev_jump_kernels, s));
    ASTAR_HIP(hipMemcpyAsync(h->jerr_host, h->jerr, 2 * 4, hipMemcpyDeviceToHost, s));
    ASTAR_HIP(hipEventRecord(h->ev_jump_done, s));
    h->jump_valid = true;
    h->jump_pending = true;
    return BN_OK;
}

/* Device time of the last table build's kernels, in ms: for the rate tool. */
int bn_astar_jump_ms(bn_astar_t *h, float *ms)
{
    if (!h || !ms) return astar_fail(BN_ERR_INVALID, "null argument");
    ASTAR_ON_DEVICE(h);
    int rc = jump_ready(h);
    if (rc != BN_OK) return rc;
    ASTAR_HIP(hipEventElapsedTime(ms, h->ev_jump_start, h->ev_jump_kernels));
    return BN_OK;
}

int bn_astar_paths_async(bn_astar_t *h, int32_t inst, const int32_t *starts_xy, bn_mem_kind where, int32_t n, int32_t max_len,
                         int32_t *out_xy_device, int32_t *out_len_device, void *stream)
{
    if (!h) return astar_fail(BN_ERR_INVALID, "null handle");
    if (inst < 0 || inst >= h->B) return astar_fail(BN_ERR_INVALID, "instance out of range");
    if (n < 0 || max_len < 0) return astar_fail(BN_ERR_INVALID, "n and max_len must be >= 0");
    if (where != BN_MEM_HOST && where != BN_MEM_DEVICE) return astar_fail(BN_ERR_INVALID, "unknown memory kind");
    ASTAR_ON_DEVICE(h);
    int rc = jump_ready(h);
    if (rc != BN_OK) return rc;
    if (n == 0) return BN_OK;
    if (!starts_xy || !out_len_device || (max_len > 0 && !out_xy_device)) return astar_fail(BN_ERR_INVALID, "null argument");
    const size_t threads = (size_t)n * (max_len > 0 ? max_len : 1);
    if (threads > ((size_t)1 << 31) * 256) return astar_fail(BN_ERR_INVALID, "n * max_len is too large for one launch");
    hipStream_t s = (hipStream_t)stream;
    const int32_t *starts = starts_xy;
    if (where == BN_MEM_HOST) {
        wait_readers(h);                          // an earlier call's kernel may still read the staging buffer
        if ((size_t)n > h->starts_cap) {
            h->starts_cap = 0;
            if ((rc = h->bufs.resize(&h->starts_dev, (size_t)n * 2 * 4, astar_fail))) return rc;
            h->starts_cap = (size_t)n;
        }
        ASTAR_HIP(hipMemcpyAsync(h->starts_dev, starts_xy, (size_t)n * 2 * 4, hipMemcpyHostToDevice, s));
        ASTAR_HIP(hipStreamSynchronize(s));       // (pageable source: the caller's buffer is free on return)
        starts = h->starts_dev;
    }
    ASTAR_HIP(hipStreamWaitEvent(s, h->ev_jump_kernels, 0));
    const size_t cells = (size_t)h->H * h->W;
    bn::PathsArgs a{h->hopbuf[0] + cells * inst, h->jump + cells * h->levels * inst, starts, out_xy_device, out_len_device,
                    h->H, h->W, n, max_len};
    bn::astar_paths_kernel<<<(unsigned)((threads + 255) / 256), 256, 0, s>>>(a);
    ASTAR_HIP(hipGetLastError());
    return bn::astar_add_reader(h, s);
}

/* Test hook: the device tables of instance `inst` -- hops (H*W int32) and jump (levels, H*W int32).  Valid after a build and
 * bn_astar_sync. */
int bn_astar_jump_buffers(bn_astar_t *h, int32_t inst, void **hops_dev, void **jump_dev, int32_t *levels, int32_t *elem_bytes)
{
    if (!h || !hops_dev || !jump_dev || !levels || !elem_bytes) return astar_fail(BN_ERR_INVALID, "null argument");
    if (inst < 0 || inst >= h->B) return astar_fail(BN_ERR_INVALID, "instance out of range");
    if (!h->jump) return astar_fail(BN_ERR_STATE, "the jump tables were never built");
    const size_t cells = (size_t)h->H * h->W;
    *hops_dev = h->hopbuf[0] + cells * inst;
    *jump_dev = h->jump + cells * h->levels * inst;
    *levels = h->levels;
    *elem_bytes = 4;
    return BN_OK;
}

}  // extern "C"

namespace bn {

int astar_view(bn_astar_t *h, AStarView *v)
{
    if (!h || !v) return astar_fail(BN_ERR_INVALID, "null argument");
    if (!h->solved) return astar_fail(BN_ERR_STATE, "no A* solve has been enqueued");
    *v = AStarView{h->device, h->H, h->W, h->B, h->next, h->risk, h->inst_dev, h->ctl + 1, h->ev_kernels,
                   h->jump_valid, h->levels, h->hopbuf[0], h->jump, h->jerr, h->ev_jump_kernels};
    return BN_OK;
}

int astar_add_reader(bn_astar_t *h, hipStream_t s)
{
    ASTAR_ON_DEVICE(h);
    // one event stands for every reader: `s` waits, on the device, for the readers another stream enqueued before it is re-recorded
    if (h->reader_pending && h->reader_stream != s) ASTAR_HIP(hipStreamWaitEvent(s, h->ev_reader, 0));
    ASTAR_HIP(hipEventRecord(h->ev_reader, s));
    h->reader_pending = true;
    h->reader_stream = s;
    return BN_OK;
}

}  // namespace bn
