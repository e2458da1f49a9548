// The RRT global planner for B instances per launch: `RRT` and `Tree` of the reference
// (src/planners/global_planners/sampling_based/{rrt,tree}.py) on the device, bit for bit.  One workgroup per instance.
//   rrt_samples_kernel   torch's MT19937 stream of the instance (seeded, or reloaded from the handle), parsed into the sample of every
//                        iteration: one uniform u; u < f32(rate) -> the goal, else two more uniforms -> (x, y).  _steer always returns
//                        feasible, so the sample sequence does not depend on the tree.  The state goes back to the handle.
//   rrt_grow_kernel      the tree: per iteration the norm of node - sample for the n nodes across the lanes, the argmin over
//                        (distance bits, index) pairs (the lowest index wins a tie, as torch.argmin), the steer, the append.
//                        Nodes live in LDS as float2 (up to 8191 iterations: 8192 nodes, 64 KB) or in global memory.
//   rrt_path_kernel      _is_goal_reached, the pick (lowest cost, then lowest index) and _reconstruct_path.
// The norm of (dx, dy) is sqrt(fma(dy, dy, f32(dx dx))), what torch's CPU norm computes for two elements; every FMA, division and
// square root is an explicit intrinsic (-ffp-contract=off), and division and sqrt are correctly rounded (hipcc's default).
// Every index is bounded by the handle's B and iteration count: parents come out of the argmin over i < n, the stream position
// is clamped to the state block, and the path walk is bounded by the node count.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/benchnav_mppi.h"
#include "mt19937.h"
#include "rrt_device.h"

namespace bn {
namespace {

constexpr int kRrtSampleThreads = 256;     // >= 227 (mt19937.h)
constexpr int kRrtPathThreads = 256;
constexpr int kRrtMaxWaves = 4;            // the growth kernel runs 64 or 256 threads
constexpr int kRrtLdsNodes = 8192;         // float2 nodes in 64 KB: up to 8191 iterations
constexpr int kRrtResult = 4;              // found, picked node, path length, near-goal count

struct RrtSampleArgs {
    const uint64_t *seeds;     // (B), read when reseed
    uint32_t *state;           // (B, 624) the block of the stream being read
    int32_t *pos;              // (B) the next word in it, 624 = twist first
    const float *goals;        // (B, 2)
    float *samples;            // (B, iters, 2)
    int32_t *flags;            // (B, iters) 1 where the sample is the goal
    int iters, reseed;
    float rate, xspan, x0, yspan, y0;      // f32(rate), f32(x1 - x0), f32(x0), f32(y1 - y0), f32(y0)
};

__global__ __launch_bounds__(kRrtSampleThreads) void rrt_samples_kernel(RrtSampleArgs a)
{
    __shared__ uint32_t mt[2][kMtN];
    const int b = blockIdx.x, t = threadIdx.x;
    int pos = kMtN;
    if (a.reseed) {
        if (t == 0) mt_seed(mt[0], (uint32_t)a.seeds[b]);
    } else {
        for (int i = t; i < kMtN; i += kRrtSampleThreads) mt[0][i] = a.state[(size_t)b * kMtN + i];
        pos = min(max(a.pos[b], 0), kMtN);
    }
    __syncthreads();
    MtStream s{mt, 0, pos};
    const float gx = a.goals[2 * b], gy = a.goals[2 * b + 1];
    float *out = a.samples + (size_t)b * a.iters * 2;
    int32_t *fl = a.flags + (size_t)b * a.iters;
    // every thread walks the same words (the parse is a dependent chain: 1 or 3 draws per iteration); they take turns to write
    for (int it = 0; it < a.iters; ++it) {
        const bool goal = mt_next(s) < a.rate;
        float x = gx, y = gy;
        if (!goal) {
            x = __fadd_rn(__fmul_rn(mt_next(s), a.xspan), a.x0);
            y = __fadd_rn(__fmul_rn(mt_next(s), a.yspan), a.y0);
        }
        if (t == (it & (kRrtSampleThreads - 1))) {
            out[2 * it] = x;
            out[2 * it + 1] = y;
            fl[it] = goal ? 1 : 0;
        }
    }
    for (int i = t; i < kMtN; i += kRrtSampleThreads) a.state[(size_t)b * kMtN + i] = s.mt[s.cur][i];
    if (t == 0) a.pos[b] = s.pos;
}

struct RrtGrowArgs {
    const float *starts;       // (B, 2)
    const float *samples;      // (B, iters, 2)
    float2 *nodes;             // (B, cap, 2)
    int32_t *edges;            // (B, cap)
    float *costs;              // (B, cap)
    int32_t *counts;           // (B)
    int iters, cap;            // cap = iters + 1
    int lds_costs;             // LDS nodes only: the costs sit behind the nodes in LDS too
    float delta;               // f32(delta_distance)
};

template <int THREADS, bool LDS_NODES>
__global__ __launch_bounds__(THREADS) void rrt_grow_kernel(RrtGrowArgs a)
{
    extern __shared__ float2 lnodes[];                       // LDS_NODES: cap nodes, then (lds_costs) cap costs
    __shared__ unsigned long long part[kRrtMaxWaves];
    const int b = blockIdx.x, t = threadIdx.x;
    float2 *gnodes = a.nodes + (size_t)b * a.cap;
    int32_t *edges = a.edges + (size_t)b * a.cap;
    float *gcosts = a.costs + (size_t)b * a.cap;
    float *lcosts = (float *)(lnodes + a.cap);
    const float *samp = a.samples + (size_t)b * a.iters * 2;
    if (t == 0) {
        const float2 s0 = make_float2(a.starts[2 * b], a.starts[2 * b + 1]);
        gnodes[0] = s0;
        edges[0] = -1;
        gcosts[0] = 0.0f;
        if (LDS_NODES) {
            lnodes[0] = s0;
            if (a.lds_costs) lcosts[0] = 0.0f;
        }
    }
    float nsx = 0.0f, nsy = 0.0f;
    if (a.iters > 0) { nsx = samp[0]; nsy = samp[1]; }
    __syncthreads();
    for (int it = 0; it < a.iters; ++it) {
        const int n = it + 1;
        const float sx = nsx, sy = nsy;
        if (it + 1 < a.iters) { nsx = samp[2 * it + 2]; nsy = samp[2 * it + 3]; }      // the next sample, off the critical path
        // Tree.nearest_neighbor: argmin of norm(node - sample) over the n nodes.  Distances are >= +0, so their bit patterns order
        // as unsigned integers; the index in the low word makes the lowest index win among equal distances.
        unsigned long long key = ~0ull;
        for (int i = t; i < n; i += THREADS) {
            const float2 p = LDS_NODES ? lnodes[i] : gnodes[i];
            const float d = rrt_norm(__fsub_rn(p.x, sx), __fsub_rn(p.y, sy));
            const unsigned long long k = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)i;
            key = k < key ? k : key;
        }
        key = block_min_u64<THREADS>(key, part);
        const int p = min((int)(unsigned)(key & 0xffffffffu), it);                    // thread 0 always offers node 0: p < n
        // _steer, by every thread on the same values; thread 0 appends
        const float2 f = LDS_NODES ? lnodes[p] : gnodes[p];
        float dx = __fsub_rn(sx, f.x), dy = __fsub_rn(sy, f.y);
        float d = rrt_norm(dx, dy);
        if (d > a.delta) {
            dx = __fmul_rn(__fdiv_rn(dx, d), a.delta);
            dy = __fmul_rn(__fdiv_rn(dy, d), a.delta);
            d = a.delta;
        }
        if (t == 0) {
            const float2 nn = make_float2(__fadd_rn(f.x, dx), __fadd_rn(f.y, dy));
            const float c = __fadd_rn((LDS_NODES && a.lds_costs) ? lcosts[p] : gcosts[p], d);
            gnodes[n] = nn;
            edges[n] = p;
            gcosts[n] = c;
            if (LDS_NODES) {
                lnodes[n] = nn;
                if (a.lds_costs) lcosts[n] = c;
            }
        }
        __syncthreads();                                                               // the new node is there for every lane
    }
    if (t == 0) a.counts[b] = a.iters + 1;
}

struct RrtPathArgs {
    const float2 *nodes;
    const int32_t *edges;
    const float *costs;
    const float *goals;        // (B, 2)
    float2 *paths;             // (B, path_cap, 2), NaN beyond the path
    int32_t *results;          // (B, kRrtResult)
    int n, cap, path_cap;
    float threshold;           // f32(goal_threshold)
};

__global__ __launch_bounds__(kRrtPathThreads) void rrt_path_kernel(RrtPathArgs a)
{
    __shared__ unsigned long long part[kRrtMaxWaves];
    __shared__ int cnt[kRrtMaxWaves];
    __shared__ int length;
    const int b = blockIdx.x, t = threadIdx.x;
    const float2 *nodes = a.nodes + (size_t)b * a.cap;
    const int32_t *edges = a.edges + (size_t)b * a.cap;
    const float *costs = a.costs + (size_t)b * a.cap;
    float2 *path = a.paths + (size_t)b * a.path_cap;
    const float gx = a.goals[2 * b], gy = a.goals[2 * b + 1];
    // _is_goal_reached: nodes with norm(node - goal) < f32(threshold); among them the lowest cost, then the lowest index
    // (costs are >= +0: their bit patterns order as unsigned integers)
    unsigned long long key = ~0ull;
    int near = 0;
    for (int i = t; i < a.n; i += kRrtPathThreads) {
        const float2 p = nodes[i];
        if (rrt_norm(__fsub_rn(p.x, gx), __fsub_rn(p.y, gy)) < a.threshold) {
            ++near;
            const unsigned long long k = ((unsigned long long)__float_as_uint(costs[i]) << 32) | (unsigned)i;
            key = k < key ? k : key;
        }
    }
    for (int m = 32; m > 0; m >>= 1) near += __shfl_xor(near, m, 64);
    if ((t & 63) == 0) cnt[t >> 6] = near;
    key = block_min_u64<kRrtPathThreads>(key, part);                                   // its barrier covers cnt[] too
    if (t == 0) {
        int total = 0;
        for (int w = 0; w < kRrtPathThreads / 64; ++w) total += cnt[w];
        int32_t *res = a.results + (size_t)b * kRrtResult;
        int L = 0, pick = -1;
        if (total > 0) {
            pick = min((int)(unsigned)(key & 0xffffffffu), a.n - 1);
            // _reconstruct_path: follow the parents to node 0 (a parent has a lower index than its child), then write root first
            L = 1;
            for (int cur = pick; cur != 0 && L <= a.n; ++L) cur = min(max(edges[cur], 0), a.n - 1);
            int k = L - 1;
            for (int cur = pick; k >= 0; --k) {
                if (k < a.path_cap) path[k] = nodes[cur];
                cur = min(max(edges[cur], 0), a.n - 1);                                // the root's -1 is read last and not used
            }
        }
        res[0] = total > 0; res[1] = pick; res[2] = L; res[3] = total;
        length = L;
    }
    __syncthreads();
    for (int i = length + t; i < a.path_cap; i += kRrtPathThreads) path[i] = make_float2(NAN, NAN);
}

thread_local std::string g_rrt_error;

}  // namespace
}  // namespace bn

struct bn_rrt {
    bn_rrt_config cfg{};
    int B = 0, iters = 0, cap = 0, path_cap = 0, threads = 256;
    bool lds_nodes = true, lds_costs = false, seeded = false, ev_recorded = false;
    size_t lds_bytes = 0;
    float2 *nodes = nullptr, *paths = nullptr;
    int32_t *edges = nullptr, *counts = nullptr, *flags = nullptr, *results = nullptr, *pos = nullptr;
    float *costs = nullptr, *samples = nullptr, *starts = nullptr, *goals = nullptr;
    uint32_t *state = nullptr;
    uint64_t *seeds = nullptr;
    unsigned char *pinned = nullptr;         // staging: starts (B, 2), goals (B, 2) float32, then seeds (B) uint64
    hipEvent_t ev_done = nullptr;
};

namespace {

int rrt_fail(int code, const std::string &msg)
{
    bn::g_rrt_error = msg;
    return code;
}

struct RrtDeviceGuard {
    int prev = -1; bool changed = false, ok = true;
    explicit RrtDeviceGuard(int want) { if (hipGetDevice(&prev) != hipSuccess) { ok = false; return; }
                                        if (prev != want) { ok = hipSetDevice(want) == hipSuccess; changed = ok; } }
    ~RrtDeviceGuard() { if (changed) (void)hipSetDevice(prev); }
};

#define RRT_HIP(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return rrt_fail(BN_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

template <typename P>
int rrt_alloc(P **p, size_t bytes)
{
    RRT_HIP(hipMalloc((void **)p, bytes ? bytes : 4));
    RRT_HIP(hipMemset(*p, 0, bytes ? bytes : 4));
    return BN_OK;
}

bool in_bounds(const bn_rrt_config &c, const float *p)
{
    // RRT._is_within_bounds: x0 <= x <= x1 and y0 <= y <= y1 on the float32 position (NaN fails)
    return c.x_limits[0] <= (double)p[0] && (double)p[0] <= c.x_limits[1] && c.y_limits[0] <= (double)p[1] && (double)p[1] <= c.y_limits[1];
}

int check_positions(const bn_rrt_t *h, const float *starts, const float *goals)
{
    for (int b = 0; b < h->B; ++b)
        if (!in_bounds(h->cfg, starts + 2 * b) || !in_bounds(h->cfg, goals + 2 * b))
            return rrt_fail(BN_ERR_INVALID, "Start or goal position is out of bounds (instance " + std::to_string(b) + ")");
    return BN_OK;
}

// starts and goals through the pinned staging block onto the stream (the caller's arrays are consumed before this returns)
int stage_positions(bn_rrt_t *h, const float *starts, const float *goals, hipStream_t s)
{
    if (h->ev_recorded) RRT_HIP(hipEventSynchronize(h->ev_done));                       // the staging block is free again
    const size_t pb = (size_t)h->B * 8;
    std::memcpy(h->pinned, starts, pb);
    std::memcpy(h->pinned + pb, goals, pb);
    RRT_HIP(hipMemcpyAsync(h->starts, h->pinned, pb, hipMemcpyHostToDevice, s));
    RRT_HIP(hipMemcpyAsync(h->goals, h->pinned + pb, pb, hipMemcpyHostToDevice, s));
    return BN_OK;
}

template <int THREADS>
void launch_grow(const bn_rrt_t *h, const bn::RrtGrowArgs &a, hipStream_t s)
{
    if (h->lds_nodes) bn::rrt_grow_kernel<THREADS, true><<<h->B, THREADS, h->lds_bytes, s>>>(a);
    else bn::rrt_grow_kernel<THREADS, false><<<h->B, THREADS, 0, s>>>(a);
}

// the growth and the goal test / pick / path on the handle's sample table
int grow_and_pick(bn_rrt_t *h, hipStream_t s)
{
    bn::RrtGrowArgs g{};
    g.starts = h->starts; g.samples = h->samples; g.nodes = h->nodes; g.edges = h->edges; g.costs = h->costs; g.counts = h->counts;
    g.iters = h->iters; g.cap = h->cap; g.lds_costs = h->lds_costs; g.delta = (float)h->cfg.delta_distance;
    if (h->threads == 64) launch_grow<64>(h, g, s);
    else launch_grow<256>(h, g, s);
    RRT_HIP(hipGetLastError());
    bn::RrtPathArgs p{};
    p.nodes = h->nodes; p.edges = h->edges; p.costs = h->costs; p.goals = h->goals; p.paths = h->paths; p.results = h->results;
    p.n = h->cap; p.cap = h->cap; p.path_cap = h->path_cap; p.threshold = (float)h->cfg.goal_threshold;
    bn::rrt_path_kernel<<<h->B, bn::kRrtPathThreads, 0, s>>>(p);
    RRT_HIP(hipGetLastError());
    RRT_HIP(hipEventRecord(h->ev_done, s));
    h->ev_recorded = true;
    return BN_OK;
}

}  // namespace

extern "C" {

const char *bn_rrt_last_error(void) { return bn::g_rrt_error.c_str(); }

void bn_rrt_config_init(bn_rrt_config *cfg)
{
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = (uint32_t)sizeof(*cfg);
    cfg->num_instances = 1;
    cfg->max_iterations = 1000;              // rrt.py:34-39
    cfg->path_cap = 0;                       // 0: max_iterations + 1, the longest path there can be
    cfg->x_limits[0] = 0.0; cfg->x_limits[1] = 32.0;
    cfg->y_limits[0] = 0.0; cfg->y_limits[1] = 32.0;
    cfg->delta_distance = 5.0;
    cfg->goal_sample_rate = 0.1;
    cfg->goal_threshold = 0.1;               // _is_goal_reached's default
    cfg->seed = 42;
}

int bn_rrt_create(const bn_rrt_config *cfg, bn_rrt_t **out)
{
    if (!out) return rrt_fail(BN_ERR_INVALID, "null handle pointer");
    *out = nullptr;
    if (!cfg) return rrt_fail(BN_ERR_INVALID, "null config");
    if (cfg->struct_size != sizeof(bn_rrt_config)) return rrt_fail(BN_ERR_INVALID, "bn_rrt_config.struct_size does not match this library");
    if (cfg->num_instances < 1 || cfg->max_iterations < 1 || cfg->max_iterations > (1 << 20) ||
        (int64_t)cfg->num_instances * ((int64_t)cfg->max_iterations + 1) > ((int64_t)1 << 27))
        return rrt_fail(BN_ERR_INVALID, "num_instances >= 1, max_iterations in [1, 2^20], and their product must fit 2^27 nodes");
    if (cfg->path_cap < 0 || cfg->path_cap > cfg->max_iterations + 1) return rrt_fail(BN_ERR_INVALID, "path_cap must be in [0, max_iterations + 1]");
    for (double v : {cfg->x_limits[0], cfg->x_limits[1], cfg->y_limits[0], cfg->y_limits[1], cfg->delta_distance, cfg->goal_sample_rate, cfg->goal_threshold})
        if (!std::isfinite(v)) return rrt_fail(BN_ERR_INVALID, "limits, delta_distance, goal_sample_rate and goal_threshold must be finite");
    if (!(cfg->x_limits[1] >= cfg->x_limits[0]) || !(cfg->y_limits[1] >= cfg->y_limits[0])) return rrt_fail(BN_ERR_INVALID, "limits must be ordered");
    if (cfg->seed > 0xFFFFFFFFull) return rrt_fail(BN_ERR_INVALID, "Seed must be between 0 and 2**32 - 1");
    if ((cfg->flags & BN_RRT_FLAG_ONE_WAVE) && (cfg->flags & BN_RRT_FLAG_FOUR_WAVES)) return rrt_fail(BN_ERR_INVALID, "one workgroup size at a time");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return rrt_fail(BN_ERR_NO_DEVICE, "no HIP device visible: no CPU fallback");
    if (cfg->device_id < 0 || cfg->device_id >= ndev) return rrt_fail(BN_ERR_INVALID, "device_id out of range");
    RrtDeviceGuard guard(cfg->device_id);
    if (!guard.ok) return rrt_fail(BN_ERR_HIP, "hipSetDevice failed");
    auto *h = new bn_rrt_t();
    h->cfg = *cfg;
    h->B = cfg->num_instances; h->iters = cfg->max_iterations; h->cap = h->iters + 1;
    h->path_cap = cfg->path_cap ? cfg->path_cap : h->cap;
    h->threads = (cfg->flags & BN_RRT_FLAG_ONE_WAVE) ? 64 : 256;                          // 256 is the faster one
    h->lds_nodes = !(cfg->flags & BN_RRT_FLAG_GLOBAL_NODES) && h->cap <= bn::kRrtLdsNodes;
    h->lds_costs = h->lds_nodes && (size_t)h->cap * 12 <= (size_t)bn::kRrtLdsNodes * 8;
    h->lds_bytes = h->lds_nodes ? (size_t)h->cap * (h->lds_costs ? 12 : 8) : 0;
    const size_t B = h->B, nc = B * h->cap, ni = B * h->iters;
    int rc = BN_OK;
    if ((rc = rrt_alloc(&h->nodes, nc * 8)) || (rc = rrt_alloc(&h->edges, nc * 4)) || (rc = rrt_alloc(&h->costs, nc * 4)) ||
        (rc = rrt_alloc(&h->counts, B * 4)) || (rc = rrt_alloc(&h->samples, ni * 8)) || (rc = rrt_alloc(&h->flags, ni * 4)) ||
        (rc = rrt_alloc(&h->paths, B * h->path_cap * 8)) || (rc = rrt_alloc(&h->results, B * bn::kRrtResult * 4)) ||
        (rc = rrt_alloc(&h->state, B * bn::kMtN * 4)) || (rc = rrt_alloc(&h->pos, B * 4)) || (rc = rrt_alloc(&h->starts, B * 8)) ||
        (rc = rrt_alloc(&h->goals, B * 8)) || (rc = rrt_alloc(&h->seeds, B * 8))) {
        std::string keep = bn::g_rrt_error;
        bn_rrt_destroy(h);
        bn::g_rrt_error = keep;
        return rc;
    }
    if (hipHostMalloc((void **)&h->pinned, B * 24, hipHostMallocDefault) != hipSuccess || hipEventCreate(&h->ev_done) != hipSuccess) {
        bn_rrt_destroy(h);
        return rrt_fail(BN_ERR_HIP, "RRT handle initialisation failed");
    }
    *out = h;
    return BN_OK;
}

void bn_rrt_destroy(bn_rrt_t *h)
{
    if (!h) return;
    RrtDeviceGuard guard(h->cfg.device_id);
    if (h->ev_recorded && h->ev_done) (void)hipEventSynchronize(h->ev_done);
    for (void *p : {(void *)h->nodes, (void *)h->edges, (void *)h->costs, (void *)h->counts, (void *)h->samples, (void *)h->flags,
                    (void *)h->paths, (void *)h->results, (void *)h->state, (void *)h->pos, (void *)h->starts, (void *)h->goals,
                    (void *)h->seeds})
        if (p) (void)hipFree(p);
    if (h->pinned) (void)hipHostFree(h->pinned);
    if (h->ev_done) (void)hipEventDestroy(h->ev_done);
    delete h;
}

int bn_rrt_plan_async(bn_rrt_t *h, void *stream, const float *starts, const float *goals, const uint64_t *seeds)
{
    if (!h || !starts || !goals) return rrt_fail(BN_ERR_INVALID, "null argument");
    int rc = check_positions(h, starts, goals);
    if (rc) return rc;
    if (seeds)
        for (int b = 0; b < h->B; ++b)
            if (seeds[b] > 0xFFFFFFFFull) return rrt_fail(BN_ERR_INVALID, "Seed must be between 0 and 2**32 - 1");
    RrtDeviceGuard guard(h->cfg.device_id);
    if (!guard.ok) return rrt_fail(BN_ERR_HIP, "hipSetDevice failed");
    hipStream_t s = (hipStream_t)stream;
    if ((rc = stage_positions(h, starts, goals, s))) return rc;
    const bool reseed = seeds || !h->seeded;                  // the first plan without seeds starts every stream from the config's seed
    if (reseed) {
        uint64_t *ps = (uint64_t *)(h->pinned + (size_t)h->B * 16);
        for (int b = 0; b < h->B; ++b) ps[b] = seeds ? seeds[b] : h->cfg.seed;
        RRT_HIP(hipMemcpyAsync(h->seeds, ps, (size_t)h->B * 8, hipMemcpyHostToDevice, s));
    }
    bn::RrtSampleArgs a{};
    a.seeds = h->seeds; a.state = h->state; a.pos = h->pos; a.goals = h->goals; a.samples = h->samples; a.flags = h->flags;
    a.iters = h->iters; a.reseed = reseed;
    a.rate = (float)h->cfg.goal_sample_rate;
    a.xspan = (float)(h->cfg.x_limits[1] - h->cfg.x_limits[0]); a.x0 = (float)h->cfg.x_limits[0];
    a.yspan = (float)(h->cfg.y_limits[1] - h->cfg.y_limits[0]); a.y0 = (float)h->cfg.y_limits[0];
    bn::rrt_samples_kernel<<<h->B, bn::kRrtSampleThreads, 0, s>>>(a);
    RRT_HIP(hipGetLastError());
    h->seeded = true;
    return grow_and_pick(h, s);
}

int bn_rrt_grow_from_samples_async(bn_rrt_t *h, void *stream, const float *starts, const float *goals, const void *samples, int where)
{
    if (!h || !starts || !goals || !samples) return rrt_fail(BN_ERR_INVALID, "null argument");
    if (where != BN_MEM_HOST && where != BN_MEM_DEVICE) return rrt_fail(BN_ERR_INVALID, "where must be BN_MEM_HOST or BN_MEM_DEVICE");
    int rc = check_positions(h, starts, goals);
    if (rc) return rc;
    RrtDeviceGuard guard(h->cfg.device_id);
    if (!guard.ok) return rrt_fail(BN_ERR_HIP, "hipSetDevice failed");
    hipStream_t s = (hipStream_t)stream;
    if ((rc = stage_positions(h, starts, goals, s))) return rc;                        // waits for the handle's last launch
    const size_t bytes = (size_t)h->B * h->iters * 8;
    if (where == BN_MEM_HOST) {
        RRT_HIP(hipMemcpyAsync(h->samples, samples, bytes, hipMemcpyHostToDevice, s));
        RRT_HIP(hipStreamSynchronize(s));                                              // the caller's array is consumed before this returns
    } else {
        RRT_HIP(hipMemcpyAsync(h->samples, samples, bytes, hipMemcpyDeviceToDevice, s));
    }
    RRT_HIP(hipMemsetAsync(h->flags, 0, (size_t)h->B * h->iters * 4, s));
    return grow_and_pick(h, s);
}

int bn_rrt_sync(bn_rrt_t *h)
{
    if (!h) return rrt_fail(BN_ERR_INVALID, "null handle");
    RrtDeviceGuard guard(h->cfg.device_id);
    if (!guard.ok) return rrt_fail(BN_ERR_HIP, "hipSetDevice failed");
    if (h->ev_recorded) RRT_HIP(hipEventSynchronize(h->ev_done));
    return BN_OK;
}

int bn_rrt_device_buffer(bn_rrt_t *h, int which, void **ptr, size_t *bytes)
{
    if (!h || !ptr || !bytes) return rrt_fail(BN_ERR_INVALID, "null argument");
    const size_t B = h->B, nc = B * h->cap, ni = B * h->iters;
    switch (which) {
    case BN_RRT_BUF_NODES: *ptr = h->nodes; *bytes = nc * 8; break;
    case BN_RRT_BUF_EDGES: *ptr = h->edges; *bytes = nc * 4; break;
    case BN_RRT_BUF_COSTS: *ptr = h->costs; *bytes = nc * 4; break;
    case BN_RRT_BUF_COUNTS: *ptr = h->counts; *bytes = B * 4; break;
    case BN_RRT_BUF_SAMPLES: *ptr = h->samples; *bytes = ni * 8; break;
    case BN_RRT_BUF_SAMPLE_FLAGS: *ptr = h->flags; *bytes = ni * 4; break;
    case BN_RRT_BUF_PATHS: *ptr = h->paths; *bytes = B * h->path_cap * 8; break;
    case BN_RRT_BUF_RESULTS: *ptr = h->results; *bytes = B * bn::kRrtResult * 4; break;
    default: return rrt_fail(BN_ERR_INVALID, "unknown RRT buffer id");
    }
    return BN_OK;
}

int32_t bn_rrt_node_storage(bn_rrt_t *h) { return h ? (h->lds_nodes ? (h->lds_costs ? 2 : 1) : 0) : -1; }

}  // extern "C"
