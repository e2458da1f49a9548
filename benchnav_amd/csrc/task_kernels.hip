// task_kernels.hip -- the task stage on the device: which ground of a map is truly passable, which of it hangs
// together, and start/goal pairs drawn inside one connected region.
//
//   mask     passable[m, c] = finite(mean) && finite(std) && 1 - clamp(mean + kappa * std, 0, 1) > stuck_threshold, in float32;
//   labels   labels[m, c] = the smallest linear index iy * W + ix of c's 4- or 8-connected component, -1 on a blocked cell;
//            sizes[m, c] = the component's cells where c is such a smallest index, else 0; eight int32 of statistics per map;
//   pairs    one wave per (map, pair), 64 Philox attempts per round, the lowest accepted attempt wins.
//
// Labelling is three launches.  (1) A workgroup labels one 32 x 32 tile in LDS with a union-find whose links are atomicMin, and
// writes every cell's tile-local root as a map index into the parent array (the workspace).  (2) One wave per tile unites across
// the tile's right and lower border in that array, lock-free: a union links the LARGER root to the smaller one with atomicMin, so
// parent[x] <= x always, a chain of parents strictly falls, and the root of a set is its minimum.  Workgroups of one launch sit on
// XCDs whose L2s are not coherent: in launch (2) EVERY read and write of the parent array is an agent-scope atomic.  (3) Behind
// the kernel boundary plain loads follow the chains to the roots, write the labels and count the sizes with integer atomics.
// No kernel waits for another workgroup; every loop has a bound derived from the shape (a chain strictly falls: at most `cells`
// steps; a union lowers the sum of its two cells with every turn: at most 2 * cells turns) and a loop that reaches its bound sets
// the map's error flag and leaves.  Stateless: device pointers, the caller's stream and workspace, no allocation, no synchronisation.
#include "../../include/benchnav_mppi.h"
#include "bn_device_math.h"
#include "bn_host.h"

#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <string>

namespace bn {
namespace {

constexpr int kWave = 64;
constexpr int kThreads = 256;
constexpr int kTile = BN_TASK_TILE;                    // 32: a tile's local index fits 10 bits, lx = l & 31, ly = l >> 5
constexpr int kTileCells = kTile * kTile;
constexpr int kStats = BN_TASK_STATS;
constexpr uint32_t kTaskWord = 0x5441534Bu;            // 'TASK': the fourth counter word of every draw

typedef unsigned long long u64;

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e+38f; }      // false for NaN and +-inf

// ---- mask ----------------------------------------------------------------------------------------------------------------------
// evaluate.py's stuck(v) rule (the environment step's float32 arithmetic) on the latent slip at mean + kappa * std: a rounded
// product, then a rounded sum (-ffp-contract=off)
__global__ __launch_bounds__(kThreads) void mask_kernel(const float *__restrict__ mean, const float *__restrict__ std, int64_t total, float kappa,
                                                        float thr, uint8_t *__restrict__ mask)
{
    const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (g >= total) return;
    const float m = mean[g], s = std[g];
    const float prod = kappa * s;
    const float v = m + prod;
    mask[g] = (finite_f(m) && finite_f(s) && 1.0f - clampf(v, 0.0f, 1.0f) > thr) ? 1 : 0;
}

// ---- the union-find both labelling launches share ------------------------------------------------------------------------------
// `Mem` reads a parent and lowers one: LDS within a workgroup, agent-scope atomics on the map's parent array.
struct LdsParents {
    int *p;
    __device__ __forceinline__ int read(int x) const { return __hip_atomic_load(p + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ __forceinline__ int lower(int x, int v) const { return __hip_atomic_fetch_min(p + x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
};

struct AgentParents {
    int32_t *p;
    // astar_kernels.hip's atomic_read form: served where the atomics are, never from an XCD's own L2
    __device__ __forceinline__ int read(int x) const { return __hip_atomic_fetch_or(p + x, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ int lower(int x, int v) const { return __hip_atomic_fetch_min(p + x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

// parent[x] < x off a root: at most `bound` steps
template <typename Mem>
__device__ __forceinline__ int find_root(const Mem &mem, int x, int bound, bool *overrun)
{
    for (int i = 0; i < bound; ++i) {
        const int p = mem.read(x);
        if (p == x) return x;
        x = p;
    }
    *overrun = true;
    return x;
}

// Unites the sets of a and b.  The larger root a is linked to the smaller root b with atomicMin.  Where a was no root any more
// (another thread linked it to `old` < a in between) parent[a] is now min(old, b): the link that lost is made good by uniting old
// with b, which this thread goes on to do.  Every such turn replaces a by a smaller cell: at most 2 * bound turns.
template <typename Mem>
__device__ __forceinline__ void unite(const Mem &mem, int a, int b, int bound, bool *overrun)
{
    for (int64_t i = 0; i < 2 * (int64_t)bound; ++i) {
        a = find_root(mem, a, bound, overrun);
        b = find_root(mem, b, bound, overrun);
        if (*overrun || a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = mem.lower(a, b);
        if (old == a) return;
        a = old;
    }
    *overrun = true;
}

struct TileOf {
    int64_t map;
    int tx, ty;
    __device__ TileOf(int64_t bid, int TX, int TY)
    {
        const int64_t tiles = (int64_t)TX * TY;
        map = bid / tiles;
        const int t = (int)(bid - map * tiles);
        ty = t / TX;
        tx = t - ty * TX;
    }
};

// ---- labels 1: a tile to its local fixpoint in LDS -----------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void tile_label_kernel(const uint8_t *__restrict__ mask, int H, int W, int TX, int TY, int conn8,
                                                              int32_t *__restrict__ parent, int32_t *__restrict__ stats)
{
    __shared__ int lp[kTileCells];
    const TileOf t(blockIdx.x, TX, TY);
    const size_t base = (size_t)t.map * (size_t)H * (size_t)W;
    const int x0 = t.tx * kTile, y0 = t.ty * kTile;
    for (int l = threadIdx.x; l < kTileCells; l += kThreads) {
        const int x = x0 + (l & (kTile - 1)), y = y0 + (l >> 5);
        lp[l] = (x < W && y < H && mask[base + (size_t)y * W + x]) ? l : -1;       // a cell off the map is blocked
    }
    __syncthreads();
    const LdsParents mem{lp};
    bool overrun = false;
    for (int l = threadIdx.x; l < kTileCells; l += kThreads) {
        if (mem.read(l) < 0) continue;
        const int lx = l & (kTile - 1), ly = l >> 5;
        if (lx < kTile - 1 && mem.read(l + 1) >= 0) unite(mem, l, l + 1, kTileCells, &overrun);
        if (ly < kTile - 1) {
            if (mem.read(l + kTile) >= 0) unite(mem, l, l + kTile, kTileCells, &overrun);
            if (conn8) {
                if (lx > 0 && mem.read(l + kTile - 1) >= 0) unite(mem, l, l + kTile - 1, kTileCells, &overrun);
                if (lx < kTile - 1 && mem.read(l + kTile + 1) >= 0) unite(mem, l, l + kTile + 1, kTileCells, &overrun);
            }
        }
    }
    __syncthreads();
    // the local index orders a tile's cells as the map index does: the local root is the component's smallest map index in the tile
    for (int l = threadIdx.x; l < kTileCells; l += kThreads) {
        const int x = x0 + (l & (kTile - 1)), y = y0 + (l >> 5);
        if (x >= W || y >= H) continue;
        int out = -1;
        if (mem.read(l) >= 0) {
            const int r = find_root(mem, l, kTileCells, &overrun);
            out = (y0 + (r >> 5)) * W + x0 + (r & (kTile - 1));
        }
        parent[base + (size_t)y * W + x] = out;
    }
    if (overrun) atomicOr(&stats[t.map * kStats + 4], BN_TASK_ERR_TILE);
}

// ---- labels 2: unions across tile borders, agent-scope atomics only ------------------------------------------------------------
// One wave per tile.  Lanes 0-31 own the cells of the tile's right column and look at the three cells right of it, lanes 32-63 the
// lower row and the three cells below: every pair of neighbours in different tiles is seen from the left or from above.
__global__ __launch_bounds__(kWave) void border_unite_kernel(const uint8_t *__restrict__ mask, int H, int W, int TX, int TY, int conn8,
                                                             int32_t *parent, int32_t *__restrict__ stats)
{
    const TileOf t(blockIdx.x, TX, TY);
    const size_t base = (size_t)t.map * (size_t)H * (size_t)W;
    const int lane = threadIdx.x, k = lane & (kTile - 1);
    const bool column = lane < kTile;
    const int x = t.tx * kTile + (column ? kTile - 1 : k), y = t.ty * kTile + (column ? k : kTile - 1);
    if (x >= W || y >= H || !mask[base + (size_t)y * W + x]) return;
    const AgentParents mem{parent + base};
    const int cells = H * W;                           // <= 2^24
    bool overrun = false;
    for (int d = -1; d <= 1; ++d) {
        if (d != 0 && !conn8) continue;
        const int nx = column ? x + 1 : x + d, ny = column ? y + d : y + 1;
        if (nx < 0 || nx >= W || ny < 0 || ny >= H || !mask[base + (size_t)ny * W + nx]) continue;
        unite(mem, y * W + x, ny * W + nx, cells, &overrun);
    }
    if (overrun) atomicOr(&stats[t.map * kStats + 4], BN_TASK_ERR_UNITE);
}

// ---- labels 3: flatten and count -----------------------------------------------------------------------------------------------
// Behind the kernel boundary the parent array is read-only: plain loads.  A wave adds the cells that share a root with one atomic.
__global__ __launch_bounds__(kThreads) void flatten_kernel(const int32_t *__restrict__ parent, int64_t cells, int64_t total,
                                                           int32_t *__restrict__ labels, int32_t *__restrict__ sizes, int32_t *__restrict__ stats)
{
    const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    int64_t key = -1;                                  // map * cells + root
    if (g < total) {
        const int64_t map = g / cells;
        const int32_t *P = parent + map * cells;
        int x = P[g - map * cells];
        if (x >= 0) {
            bool rooted = false;
            for (int64_t i = 0; i < cells; ++i) {
                const int p = P[x];
                if (p == x) { rooted = true; break; }
                x = p;
            }
            if (!rooted) atomicOr(&stats[map * kStats + 4], BN_TASK_ERR_FLATTEN);
            key = map * cells + x;
        }
        labels[g] = x;                                 // -1 on a blocked cell
    }
    u64 todo = __ballot(key >= 0);
    while (todo) {                                     // wave-uniform: one turn per root present in these 64 cells
        const int leader = __ffsll((long long)todo) - 1;
        const int64_t lk = __shfl(key, leader, kWave);
        const u64 members = __ballot(key == lk);
        if (lane == leader) atomicAdd(&sizes[lk], (int32_t)__popcll(members));
        todo &= ~members;
    }
}

// ---- statistics: one workgroup per map ------------------------------------------------------------------------------------------
// the largest component as one 64-bit maximum: (size, then the smaller label) = size << 32 | ~label
__global__ __launch_bounds__(kThreads) void stats_kernel(const int32_t *__restrict__ sizes, int64_t cells, int32_t *__restrict__ stats)
{
    __shared__ u64 s_best[kThreads / kWave];
    __shared__ int64_t s_cells[kThreads / kWave];
    __shared__ int32_t s_comps[kThreads / kWave];
    const int32_t *S = sizes + (int64_t)blockIdx.x * cells;
    u64 best = 0;
    int64_t passable = 0;
    int32_t comps = 0;
    for (int64_t c = threadIdx.x; c < cells; c += kThreads) {
        const int32_t n = S[c];
        if (n > 0) {
            const u64 k = ((u64)(uint32_t)n << 32) | (u64)(0xFFFFFFFFu - (uint32_t)c);
            best = k > best ? k : best;
            passable += n;
            ++comps;
        }
    }
    for (int off = kWave / 2; off >= 1; off >>= 1) {
        const u64 ob = __shfl_xor(best, off, kWave);
        best = ob > best ? ob : best;
        passable += __shfl_xor(passable, off, kWave);
        comps += __shfl_xor(comps, off, kWave);
    }
    const int wave = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) { s_best[wave] = best; s_cells[wave] = passable; s_comps[wave] = comps; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kThreads / kWave; ++w) {
            best = s_best[w] > best ? s_best[w] : best;
            passable += s_cells[w];
            comps += s_comps[w];
        }
        int32_t *out = stats + (int64_t)blockIdx.x * kStats;
        out[0] = (int32_t)passable;
        out[1] = comps;
        out[2] = (int32_t)(best >> 32);
        out[3] = best ? (int32_t)(0xFFFFFFFFu - (uint32_t)best) : -1;
        // out[4]: the error flags the labelling launches set; out[5..7] stay the zeros the memset left
    }
}

// ---- pairs ---------------------------------------------------------------------------------------------------------------------
struct SampleArgs {
    const int32_t *labels, *sizes;
    int32_t *cells, *attempt;
    float *positions;
    int H, W, P, border, min_component, max_attempts;
    int64_t min_sep_sq;
    uint32_t k0, k1, first_map;
    float x0, y0, res;
};

__device__ __forceinline__ float cell_centre(float origin, int i, float res)
{
    const float half = (float)i + 0.5f;                // exact: i < 2^23
    const float off = half * res;
    return origin + off;
}

// one wave per (map, pair): lane j of round k is attempt a = 64 k + j
__global__ __launch_bounds__(kWave) void sample_kernel(SampleArgs s)
{
    const int64_t map = blockIdx.x / s.P;
    const int pair = (int)(blockIdx.x - map * s.P), lane = threadIdx.x;
    const int Win = s.W - 2 * s.border, Hin = s.H - 2 * s.border;
    const uint32_t n = (uint32_t)Win * (uint32_t)Hin;
    const int64_t cells = (int64_t)s.H * s.W;
    const int32_t *L = s.labels + map * cells, *S = s.sizes + map * cells;
    int32_t *cell_out = s.cells + (size_t)blockIdx.x * 4;
    float *pos_out = s.positions + (size_t)blockIdx.x * 4;
    for (int a0 = 0; a0 < s.max_attempts; a0 += kWave) {
        const int a = a0 + lane;
        const u32x4 r = philox4x32_10(u32x4{(uint32_t)a, (uint32_t)pair, s.first_map + (uint32_t)map, kTaskWord}, s.k0, s.k1);
        const int sc = (int)__umulhi(r.x, n), gc = (int)__umulhi(r.y, n);          // < n
        const int sx = sc % Win + s.border, sy = sc / Win + s.border, gx = gc % Win + s.border, gy = gc / Win + s.border;
        const int ls = L[sy * s.W + sx], lg = L[gy * s.W + gx];
        const int64_t dx = gx - sx, dy = gy - sy;
        const bool ok = ls >= 0 && lg == ls && S[ls] >= s.min_component && dx * dx + dy * dy >= s.min_sep_sq;
        const u64 accepted = __ballot(ok);
        if (accepted) {
            if (lane == __ffsll((long long)accepted) - 1) {
                cell_out[0] = sx; cell_out[1] = sy; cell_out[2] = gx; cell_out[3] = gy;
                s.attempt[blockIdx.x] = a;
                pos_out[0] = cell_centre(s.x0, sx, s.res); pos_out[1] = cell_centre(s.y0, sy, s.res);
                pos_out[2] = cell_centre(s.x0, gx, s.res); pos_out[3] = cell_centre(s.y0, gy, s.res);
            }
            return;                                    // wave-uniform
        }
    }
    if (lane < 4) {
        cell_out[lane] = -1;
        pos_out[lane] = __uint_as_float(0x7FC00000u);
    }
    if (lane == 0) s.attempt[blockIdx.x] = -1;
}

thread_local std::string g_task_error;

int task_fail(int code, const std::string &msg)
{
    g_task_error = msg;
    return code;
}

int check_shape(int32_t M, int32_t H, int32_t W)
{
    if (M < 1 || M > BN_TASK_MAX_MAPS) return task_fail(BN_ERR_INVALID, "num_maps must be in [1, 4096]");
    if (H < 1 || H > BN_TASK_MAX_SIDE || W < 1 || W > BN_TASK_MAX_SIDE) return task_fail(BN_ERR_INVALID, "H and W must be in [1, 4096]");
    if ((int64_t)H * W > BN_TASK_MAX_CELLS) return task_fail(BN_ERR_INVALID, "H * W must be <= 2^24");
    return BN_OK;
}

}  // namespace
}  // namespace bn

extern "C" {

const char *bn_task_last_error(void) { return bn::g_task_error.c_str(); }

size_t bn_task_workspace_bytes(int32_t num_maps, int32_t H, int32_t W)
{
    if (bn::check_shape(num_maps, H, W)) return 0;
    return (size_t)num_maps * (size_t)H * (size_t)W * sizeof(int32_t);             // the parent array
}

int bn_task_mask_async(int32_t device_id, void *stream, const float *mean_device, const float *std_device, int32_t num_maps, int64_t cells,
                       float kappa, float stuck_threshold, uint8_t *mask_device)
{
    using bn::task_fail;
    if (!mean_device || !std_device) return task_fail(BN_ERR_INVALID, "null argument");
    if (!mask_device) return task_fail(BN_ERR_INVALID, "null output");
    if (num_maps < 1 || num_maps > BN_TASK_MAX_MAPS) return task_fail(BN_ERR_INVALID, "num_maps must be in [1, 4096]");
    if (cells < 1 || cells > BN_TASK_MAX_CELLS) return task_fail(BN_ERR_INVALID, "cells must be in [1, 2^24]");
    if (!std::isfinite(kappa)) return task_fail(BN_ERR_INVALID, "kappa must be finite");
    if (!std::isfinite(stuck_threshold)) return task_fail(BN_ERR_INVALID, "stuck_threshold must be finite");
    if (int rc = bn::open_device(device_id, task_fail)) return rc;
    BN_ON_DEVICE(task_fail, device_id);
    const int64_t total = (int64_t)num_maps * cells;
    bn::mask_kernel<<<(unsigned)((total + bn::kThreads - 1) / bn::kThreads), bn::kThreads, 0, (hipStream_t)stream>>>(
        mean_device, std_device, total, kappa, stuck_threshold, mask_device);
    BN_HIP_OR(task_fail, hipGetLastError());
    return BN_OK;
}

int bn_task_label_async(int32_t device_id, void *stream, const uint8_t *mask_device, int32_t num_maps, int32_t H, int32_t W,
                        int32_t connectivity, int32_t *labels_device, int32_t *sizes_device, int32_t *stats_device, void *workspace_device,
                        size_t workspace_bytes)
{
    using bn::task_fail;
    if (!mask_device) return task_fail(BN_ERR_INVALID, "null argument");
    if (!labels_device || !sizes_device || !stats_device) return task_fail(BN_ERR_INVALID, "null output");
    if (int rc = bn::check_shape(num_maps, H, W)) return rc;
    if (connectivity != 4 && connectivity != 8) return task_fail(BN_ERR_INVALID, "connectivity must be 4 or 8");
    if (!workspace_device || workspace_bytes < bn_task_workspace_bytes(num_maps, H, W))
        return task_fail(BN_ERR_INVALID, "workspace too small (bn_task_workspace_bytes)");
    if (int rc = bn::open_device(device_id, task_fail)) return rc;
    BN_ON_DEVICE(task_fail, device_id);
    hipStream_t st = (hipStream_t)stream;
    const int64_t cells = (int64_t)H * W, total = cells * num_maps;
    const int TX = (W + bn::kTile - 1) / bn::kTile, TY = (H + bn::kTile - 1) / bn::kTile, conn8 = connectivity == 8;
    const unsigned tiles = (unsigned)((int64_t)TX * TY * num_maps);                // <= 4096 * 16641 < 2^31
    int32_t *parent = (int32_t *)workspace_device;
    BN_HIP_OR(task_fail, hipMemsetAsync(sizes_device, 0, (size_t)total * sizeof(int32_t), st));
    BN_HIP_OR(task_fail, hipMemsetAsync(stats_device, 0, (size_t)num_maps * bn::kStats * sizeof(int32_t), st));
    bn::tile_label_kernel<<<tiles, bn::kThreads, 0, st>>>(mask_device, H, W, TX, TY, conn8, parent, stats_device);
    BN_HIP_OR(task_fail, hipGetLastError());
    bn::border_unite_kernel<<<tiles, bn::kWave, 0, st>>>(mask_device, H, W, TX, TY, conn8, parent, stats_device);
    BN_HIP_OR(task_fail, hipGetLastError());
    bn::flatten_kernel<<<(unsigned)((total + bn::kThreads - 1) / bn::kThreads), bn::kThreads, 0, st>>>(parent, cells, total, labels_device,
                                                                                                     sizes_device, stats_device);
    BN_HIP_OR(task_fail, hipGetLastError());
    bn::stats_kernel<<<(unsigned)num_maps, bn::kThreads, 0, st>>>(sizes_device, cells, stats_device);
    BN_HIP_OR(task_fail, hipGetLastError());
    return BN_OK;
}

int bn_task_sample_async(int32_t device_id, void *stream, const int32_t *labels_device, const int32_t *sizes_device, int32_t num_maps,
                         int32_t H, int32_t W, int32_t num_pairs, uint64_t seed, int64_t first_map, int32_t border, int64_t min_separation_sq,
                         int32_t min_component_cells, int32_t max_attempts, float x0, float y0, float resolution, int32_t *cells_device,
                         int32_t *attempt_device, float *positions_device)
{
    using bn::task_fail;
    if (!labels_device || !sizes_device) return task_fail(BN_ERR_INVALID, "null argument");
    if (!cells_device || !attempt_device || !positions_device) return task_fail(BN_ERR_INVALID, "null output");
    if (int rc = bn::check_shape(num_maps, H, W)) return rc;
    if (num_pairs < 1 || num_pairs > BN_TASK_MAX_PAIRS) return task_fail(BN_ERR_INVALID, "num_pairs must be in [1, 65536]");
    if (first_map < 0 || first_map > (int64_t)0xFFFFFFFF - num_maps) return task_fail(BN_ERR_INVALID, "first_map + num_maps must fit 32 bits");
    if (border < 0 || 2 * (int64_t)border >= (H < W ? H : W)) return task_fail(BN_ERR_INVALID, "2 * border must be < min(H, W)");
    if (min_separation_sq < 0) return task_fail(BN_ERR_INVALID, "min_separation_sq must be >= 0");
    if (min_component_cells < 0) return task_fail(BN_ERR_INVALID, "min_component_cells must be >= 0");
    if (max_attempts < bn::kWave || max_attempts > BN_TASK_MAX_ATTEMPTS || max_attempts % bn::kWave)
        return task_fail(BN_ERR_INVALID, "max_attempts must be a multiple of 64 in [64, 4096]");
    if (!std::isfinite(x0) || !std::isfinite(y0) || !std::isfinite(resolution) || !(resolution > 0.0f))
        return task_fail(BN_ERR_INVALID, "x0, y0 must be finite and resolution finite and > 0");
    if (int rc = bn::open_device(device_id, task_fail)) return rc;
    BN_ON_DEVICE(task_fail, device_id);
    const bn::SampleArgs a{labels_device, sizes_device, cells_device, attempt_device, positions_device, H, W, num_pairs, border,
                           min_component_cells, max_attempts, min_separation_sq, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)first_map,
                           x0, y0, resolution};
    bn::sample_kernel<<<(unsigned)((int64_t)num_maps * num_pairs), bn::kWave, 0, (hipStream_t)stream>>>(a);
    BN_HIP_OR(task_fail, hipGetLastError());
    return BN_OK;
}

}  // extern "C"
