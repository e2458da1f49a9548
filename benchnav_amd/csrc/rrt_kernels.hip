// The RRT global planner for B instances per launch: `RRT` and `Tree` of the reference
// (src/planners/global_planners/sampling_based/{rrt,tree}.py) on the device, bit for bit.  One workgroup per instance.
//   tree_samples_kernel<2>  (rrt_device.h) the sample of every iteration: one uniform u; u < f32(rate) -> the goal, else two more
//                        uniforms -> (x, y).  _steer always returns feasible, so the sample sequence does not depend on the tree.
//   rrt_grow_kernel      the tree: per iteration the norm of node - sample for the n nodes across the lanes, the argmin over
//                        (distance bits, index) pairs (the lowest index wins a tie, as torch.argmin), the steer, the append.
//                        Nodes live in LDS as float2 (up to 8191 iterations: 8192 nodes, 64 KB) or in global memory.
//   rrt_path_kernel      _is_goal_reached and the pick (near_goal_pick, rrt_device.h: lowest cost, then lowest index), _reconstruct_path.
// The norm of (dx, dy) is sqrt(fma(dy, dy, f32(dx dx))), what torch's CPU norm computes for two elements; every FMA, division and
// square root is an explicit intrinsic (-ffp-contract=off), and division and sqrt are correctly rounded (hipcc's default).
// Every index is bounded by the handle's B and iteration count: parents come out of the argmin over i < n, the stream position
// is clamped to the state block, and the path walk is bounded by the node count.
// The host side is written with bn_host.h (guard, HIP check, buffer table) and shares its plan steps with CL-RRT (rrt_host.h).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/benchnav_mppi.h"
#include "rrt_host.h"

namespace bn {
namespace {

constexpr int kRrtPathThreads = 256;
constexpr int kRrtMaxWaves = 4;            // the growth kernel runs 64 or 256 threads
constexpr int kRrtLdsNodes = 8192;         // float2 nodes in 64 KB: up to 8191 iterations
constexpr int kRrtResult = 4;              // found, picked node, path length, near-goal count

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
    __shared__ int length;
    const int b = blockIdx.x, t = threadIdx.x;
    const float2 *nodes = a.nodes + (size_t)b * a.cap;
    const int32_t *edges = a.edges + (size_t)b * a.cap;
    const float *costs = a.costs + (size_t)b * a.cap;
    float2 *path = a.paths + (size_t)b * a.path_cap;
    const NearGoal g = near_goal_pick<2, kRrtPathThreads>((const float *)nodes, costs, a.n, a.goals[2 * b], a.goals[2 * b + 1], a.threshold);
    if (t == 0) {
        const int total = g.total;
        int32_t *res = a.results + (size_t)b * kRrtResult;
        int L = 0, pick = -1;
        if (total > 0) {
            pick = min((int)(unsigned)(g.key & 0xffffffffu), a.n - 1);
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
    bn::DeviceBuffers bufs;                  // every device pointer below, filled by bn_rrt_create
    float2 *nodes = nullptr, *paths = nullptr;
    int32_t *edges = nullptr, *counts = nullptr, *flags = nullptr, *results = nullptr, *pos = nullptr;
    float *costs = nullptr, *samples = nullptr, *starts = nullptr, *goals = nullptr;
    uint32_t *state = nullptr;
    uint64_t *seeds = nullptr;
    unsigned char *pinned = nullptr;         // staging: starts (B, 2), goals (B, 2) float32, then seeds (B) uint64
    uint64_t *pinned_seeds = nullptr;        // ... the seeds in it
    hipEvent_t ev_done = nullptr;
};

namespace {

int rrt_fail(int code, const std::string &msg)
{
    bn::g_rrt_error = msg;
    return code;
}

#define RRT_HIP(expr) BN_HIP_AS(rrt_fail, expr, #expr)

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
    return bn::tree_mark_done(h, s, rrt_fail);
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
    if (int rc = bn::open_device(cfg->device_id, rrt_fail)) return rc;
    BN_ON_DEVICE(rrt_fail, cfg->device_id);
    auto *h = new bn_rrt_t();
    h->cfg = *cfg;
    h->B = cfg->num_instances; h->iters = cfg->max_iterations; h->cap = h->iters + 1;
    h->path_cap = cfg->path_cap ? cfg->path_cap : h->cap;
    h->threads = (cfg->flags & BN_RRT_FLAG_ONE_WAVE) ? 64 : 256;                          // 256 is the faster one
    h->lds_nodes = !(cfg->flags & BN_RRT_FLAG_GLOBAL_NODES) && h->cap <= bn::kRrtLdsNodes;
    h->lds_costs = h->lds_nodes && (size_t)h->cap * 12 <= (size_t)bn::kRrtLdsNodes * 8;
    h->lds_bytes = h->lds_nodes ? (size_t)h->cap * (h->lds_costs ? 12 : 8) : 0;
    const size_t B = h->B, nc = B * h->cap, ni = B * h->iters;
    bn::DeviceBuffers &t = h->bufs;
    t.add(&h->nodes, nc * 8, BN_RRT_BUF_NODES);
    t.add(&h->edges, nc * 4, BN_RRT_BUF_EDGES);
    t.add(&h->costs, nc * 4, BN_RRT_BUF_COSTS);
    t.add(&h->counts, B * 4, BN_RRT_BUF_COUNTS);
    t.add(&h->samples, ni * 8, BN_RRT_BUF_SAMPLES);
    t.add(&h->flags, ni * 4, BN_RRT_BUF_SAMPLE_FLAGS);
    t.add(&h->paths, B * h->path_cap * 8, BN_RRT_BUF_PATHS);
    t.add(&h->results, B * bn::kRrtResult * 4, BN_RRT_BUF_RESULTS);
    t.add(&h->state, B * bn::kMtN * 4);
    t.add(&h->pos, B * 4);
    t.add(&h->starts, B * 8);
    t.add(&h->goals, B * 8);
    t.add(&h->seeds, B * 8);
    t.add_pinned(&h->pinned, B * 24);
    t.add_event(&h->ev_done);
    if (int rc = t.alloc_all(rrt_fail)) {
        bn_rrt_destroy(h);                   // leaves the error text alone
        return rc;
    }
    h->pinned_seeds = (uint64_t *)(h->pinned + B * 16);
    *out = h;
    return BN_OK;
}

void bn_rrt_destroy(bn_rrt_t *h)
{
    if (!h) return;
    bn::DeviceGuard guard(h->cfg.device_id);
    if (h->ev_recorded && h->ev_done) (void)hipEventSynchronize(h->ev_done);
    h->bufs.free_all();
    delete h;
}

int bn_rrt_plan_async(bn_rrt_t *h, void *stream, const float *starts, const float *goals, const uint64_t *seeds)
{
    if (!h || !starts || !goals) return rrt_fail(BN_ERR_INVALID, "null argument");
    return bn::tree_plan<2>(h, stream, starts, goals, seeds, rrt_fail, grow_and_pick);
}

int bn_rrt_grow_from_samples_async(bn_rrt_t *h, void *stream, const float *starts, const float *goals, const void *samples, int where)
{
    if (!h || !starts || !goals || !samples) return rrt_fail(BN_ERR_INVALID, "null argument");
    if (where != BN_MEM_HOST && where != BN_MEM_DEVICE) return rrt_fail(BN_ERR_INVALID, "where must be BN_MEM_HOST or BN_MEM_DEVICE");
    return bn::tree_grow_from_samples<2>(h, stream, starts, goals, samples, where, rrt_fail, grow_and_pick);
}

int bn_rrt_sync(bn_rrt_t *h)
{
    if (!h) return rrt_fail(BN_ERR_INVALID, "null handle");
    BN_ON_DEVICE(rrt_fail, h->cfg.device_id);
    return bn::tree_wait_done(h, rrt_fail);
}

int bn_rrt_device_buffer(bn_rrt_t *h, int which, void **ptr, size_t *bytes)
{
    if (!h || !ptr || !bytes) return rrt_fail(BN_ERR_INVALID, "null argument");
    if (!h->bufs.find(which, ptr, bytes)) return rrt_fail(BN_ERR_INVALID, "unknown RRT buffer id");
    return BN_OK;
}

int32_t bn_rrt_node_storage(bn_rrt_t *h) { return h ? (h->lds_nodes ? (h->lds_costs ? 2 : 1) : 0) : -1; }

}  // extern "C"
