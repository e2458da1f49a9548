// rrt_host.h -- the host steps bn_rrt (rrt_kernels.hip) and bn_clrrt (clrrt_kernels.hip) share, as templates over the handle type
// and DIM, the floats per position (2: x, y; 3: x, y, heading): the position and seed checks, the staging of starts and goals
// through the handle's pinned block, the reseed upload, the sample draw, the copy-in of the caller's samples, and the ev_done
// bookkeeping.  `fail` is the family's fail function; `grow` its growth + goal test / path on the handle's sample table.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "bn_host.h"
#include "rrt_device.h"

namespace bn {
namespace {

template <typename H, typename Fail>
int tree_wait_done(H *h, Fail fail)
{
    if (h->ev_recorded) BN_HIP_OR(fail, hipEventSynchronize(h->ev_done));
    return BN_OK;
}

template <typename H, typename Fail>
int tree_mark_done(H *h, hipStream_t s, Fail fail)
{
    BN_HIP_OR(fail, hipEventRecord(h->ev_done, s));
    h->ev_recorded = true;
    return BN_OK;
}

// _is_within_bounds on the float32 positions: x0 <= x <= x1 and y0 <= y <= y1 (NaN fails); DIM == 3: finite headings
template <int DIM, typename H, typename Fail>
int tree_check_positions(const H *h, const float *starts, const float *goals, Fail fail)
{
    const auto &c = h->cfg;
    auto inside = [&c](const float *p) {
        return c.x_limits[0] <= (double)p[0] && (double)p[0] <= c.x_limits[1] && c.y_limits[0] <= (double)p[1] && (double)p[1] <= c.y_limits[1];
    };
    for (int b = 0; b < h->B; ++b) {
        if (!inside(starts + DIM * b) || !inside(goals + DIM * b))
            return fail(BN_ERR_INVALID, "Start or goal position is out of bounds (instance " + std::to_string(b) + ")");
        if (DIM == 3 && (!std::isfinite(starts[DIM * b + 2]) || !std::isfinite(goals[DIM * b + 2]))) return fail(BN_ERR_INVALID, "headings must be finite");
    }
    return BN_OK;
}

// starts and goals through the pinned staging block onto the stream (the caller's arrays are consumed before this returns)
template <int DIM, typename H, typename Fail>
int tree_stage(H *h, const float *starts, const float *goals, hipStream_t s, Fail fail)
{
    if (int rc = tree_wait_done(h, fail)) return rc;                                   // the staging block is free again
    const size_t pb = (size_t)h->B * DIM * 4;
    std::memcpy(h->pinned, starts, pb);
    std::memcpy(h->pinned + pb, goals, pb);
    BN_HIP_OR(fail, hipMemcpyAsync(h->starts, h->pinned, pb, hipMemcpyHostToDevice, s));
    BN_HIP_OR(fail, hipMemcpyAsync(h->goals, h->pinned + pb, pb, hipMemcpyHostToDevice, s));
    return BN_OK;
}

template <int DIM, typename H, typename Fail>
int tree_draw_samples(H *h, hipStream_t s, bool reseed, const int32_t *active, Fail fail)
{
    TreeSampleArgs a{};
    a.seeds = h->seeds; a.state = h->state; a.pos = h->pos; a.goals = h->goals; a.samples = h->samples; a.flags = h->flags;
    a.iters = h->iters; a.reseed = reseed; a.active = active;
    a.rate = (float)h->cfg.goal_sample_rate;
    a.xspan = (float)(h->cfg.x_limits[1] - h->cfg.x_limits[0]); a.x0 = (float)h->cfg.x_limits[0];
    a.yspan = (float)(h->cfg.y_limits[1] - h->cfg.y_limits[0]); a.y0 = (float)h->cfg.y_limits[0];
    tree_samples_kernel<DIM><<<h->B, kTreeSampleThreads, 0, s>>>(a);
    BN_HIP_OR(fail, hipGetLastError());
    return BN_OK;
}

// *_plan_async behind the family's own argument checks
template <int DIM, typename H, typename Fail, typename Grow>
int tree_plan(H *h, void *stream, const float *starts, const float *goals, const uint64_t *seeds, Fail fail, Grow grow)
{
    if (int rc = tree_check_positions<DIM>(h, starts, goals, fail)) return rc;
    if (seeds)
        for (int b = 0; b < h->B; ++b)
            if (seeds[b] > 0xFFFFFFFFull) return fail(BN_ERR_INVALID, "Seed must be between 0 and 2**32 - 1");
    BN_ON_DEVICE(fail, h->cfg.device_id);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = tree_stage<DIM>(h, starts, goals, s, fail)) return rc;
    const bool reseed = seeds || !h->seeded;                  // the first plan without seeds starts every stream from the config's seed
    if (reseed) {
        uint64_t *ps = h->pinned_seeds;
        for (int b = 0; b < h->B; ++b) ps[b] = seeds ? seeds[b] : h->cfg.seed;
        BN_HIP_OR(fail, hipMemcpyAsync(h->seeds, ps, (size_t)h->B * 8, hipMemcpyHostToDevice, s));
    }
    if (int rc = tree_draw_samples<DIM>(h, s, reseed, nullptr, fail)) return rc;
    h->seeded = true;
    return grow(h, s);
}

// *_grow_from_samples_async behind the family's own argument checks: the caller's sample table in place of the stream's
template <int DIM, typename H, typename Fail, typename Grow>
int tree_grow_from_samples(H *h, void *stream, const float *starts, const float *goals, const void *samples, int where, Fail fail, Grow grow)
{
    if (int rc = tree_check_positions<DIM>(h, starts, goals, fail)) return rc;
    BN_ON_DEVICE(fail, h->cfg.device_id);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = tree_stage<DIM>(h, starts, goals, s, fail)) return rc;                // waits for the handle's last launch
    const size_t bytes = (size_t)h->B * h->iters * DIM * 4;
    if (where == BN_MEM_HOST) {
        BN_HIP_OR(fail, hipMemcpyAsync(h->samples, samples, bytes, hipMemcpyHostToDevice, s));
        BN_HIP_OR(fail, hipStreamSynchronize(s));                                      // the caller's array is consumed before this returns
    } else {
        BN_HIP_OR(fail, hipMemcpyAsync(h->samples, samples, bytes, hipMemcpyDeviceToDevice, s));
    }
    BN_HIP_OR(fail, hipMemsetAsync(h->flags, 0, (size_t)h->B * h->iters * 4, s));
    return grow(h, s);
}

}  // namespace
}  // namespace bn
