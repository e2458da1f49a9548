// mppi_loops.cpp -- the planner loops the C ABI runs on the environment of an MPPI handle: the fused A* + DWA episode
// (astar_dwa.hip) and the CL-RRT plan-follow-replan loop (clrrt_loop.hip).
#include "mppi_handle.h"
#include "astar_dwa.h"
#include "clrrt_view.h"

#include <algorithm>
#include <cmath>
#include <vector>

using namespace bn::host;

namespace {

// The integer words of the A* + DWA loop (d_ad_i): root cell | status | status step | done step, (B) each, then the error word.
struct AdWords {
    int32_t *w;
    size_t B;
    static size_t count(size_t B) { return 4 * B + 1; }
    int32_t *root() const { return w; }
    int32_t *status() const { return w + B; }              // bn_astar_dwa_status
    int32_t *status_step() const { return status() + B; }
    int32_t *done() const { return status_step() + B; }
    int32_t *err() const { return done() + B; }
};
AdWords ad_words(const bn_mppi *h) { return AdWords{h->d_ad_i, (size_t)h->p.B}; }

// The flag words of the CL-RRT loop (d_cl_flags): (B) the replan mask, then the pending counter.
struct ClFlags {
    int32_t *w;
    size_t B;
    static size_t count(size_t B) { return B + 1; }
    int32_t *active() const { return w; }
    int32_t *pending() const { return w + B; }
};
ClFlags cl_flags(const bn_mppi *h) { return ClFlags{h->d_cl_flags, (size_t)h->p.B}; }

}  // namespace

namespace bn {
namespace host {

void loops_release(bn_mppi *h)
{
    h->ad_bufs.free_all();
    h->cl_bufs.free_all();
}

}  // namespace host
}  // namespace bn

extern "C" {

// ---- the A* + DWA closed loop (astar_dwa.hip) ----

// root cells -1, statuses BN_AD_OK, status / done steps -1, error word 0 (allocates on first use)
static int astar_dwa_clear(bn_mppi *h)
{
    const size_t B = h->p.B;
    if (h->ad_bufs.list.empty()) {
        h->ad_bufs.add(&h->d_ad_i, AdWords::count(B) * sizeof(int32_t));
        h->ad_bufs.add(&h->d_ad_state, B * 3 * sizeof(float));
        h->ad_log.attach(h->ad_bufs, B, 2);            // + the sub-goals (x, y); grows with the longest episode
    }
    if (!h->ad_bufs.live) {
        if (int rc = h->ad_bufs.ensure(table_fail)) return rc;
        if (int rc = fills_done()) return rc;
    }
    const AdWords w = ad_words(h);
    BN_HIP(hipMemsetAsync(w.root(), 0xff, B * sizeof(int32_t), h->stream));
    BN_HIP(hipMemsetAsync(w.status(), 0, B * sizeof(int32_t), h->stream));
    BN_HIP(hipMemsetAsync(w.status_step(), 0xff, 2 * B * sizeof(int32_t), h->stream));       // ... and the done steps behind them
    BN_HIP(hipMemsetAsync(w.err(), 0, sizeof(int32_t), h->stream));
    h->ad_step = 0;
    return BN_OK;
}

int bn_astar_dwa_reset(bn_mppi_t *h)
{
    if (!h) return fail(BN_ERR_INVALID, "null handle");
    BN_BIND(h);
    if (int rc = settle_point(h)) return rc;
    return astar_dwa_clear(h);
}

int bn_astar_dwa_set_root(bn_mppi_t *h, int32_t instance, int32_t ix, int32_t iy)
{
    if (!h) return fail(BN_ERR_INVALID, "null handle");
    if (instance < 0 || instance >= h->p.B) return fail(BN_ERR_INVALID, "instance out of range");
    if (ix >= 0 && (ix >= h->p.G || iy < 0 || iy >= h->p.G)) return fail(BN_ERR_INVALID, "root cell out of bounds");
    BN_BIND(h);
    if (int rc = settle_point(h)) return rc;
    if (!h->d_ad_i)
        if (int rc = astar_dwa_clear(h)) return rc;
    const int32_t cell = ix < 0 ? -1 : iy * h->p.G + ix;
    BN_HIP(hipStreamSynchronize(h->stream));
    BN_HIP(hipMemcpy(ad_words(h).root() + instance, &cell, sizeof(int32_t), hipMemcpyHostToDevice));
    return BN_OK;
}

int bn_astar_dwa_set_walk(bn_mppi_t *h, int32_t mode)
{
    if (!h) return fail(BN_ERR_INVALID, "null handle");
    if (mode != 0 && mode != 1) return fail(BN_ERR_INVALID, "walk mode must be 0 (serial) or 1 (jump tables)");
    h->ad_walk = mode;
    return BN_OK;
}

int bn_astar_dwa_episode_async(bn_mppi_t *h, bn_astar_t *a, int32_t n_steps, const float *states0, bn_mem_kind where,
                               float *prev_action_device, const float a_lim[2], float dwa_delta_t, int32_t num_lin_vel,
                               int32_t num_ang_vel, float lookahead, const float *z_device)
{
    if (!h || !a || !states0 || !prev_action_device || !a_lim) return fail(BN_ERR_INVALID, "null argument");
    if (n_steps < 1) return fail(BN_ERR_INVALID, "n_steps must be >= 1");
    const int64_t NA = (int64_t)num_lin_vel * num_ang_vel;
    if (num_lin_vel < 1 || num_ang_vel < 1 || NA > 1024) return fail(BN_ERR_INVALID, "num_lin_vel * num_ang_vel must be in [1, 1024]");
    if (where != BN_MEM_HOST && where != BN_MEM_DEVICE) return fail(BN_ERR_INVALID, "unknown memory kind");
    if (!h->env_attached) return fail(BN_ERR_STATE, "bn_mppi_env_attach must precede bn_astar_dwa_episode_async");
    if (!h->map_set || !h->goal_set) return fail(BN_ERR_STATE, "set_map and set_goal must precede bn_astar_dwa_episode_async");
    bn::AStarView v;
    if (bn::astar_view(a, &v) != BN_OK) return fail(BN_ERR_STATE, "the A* handle has no solve: bn_astar_solve_async must precede the episode");
    if (v.device != h->cfg.device_id) return fail(BN_ERR_INVALID, "the A* handle is on device %d, the planner on device %d", v.device, h->cfg.device_id);
    if (v.B != h->p.B) return fail(BN_ERR_INVALID, "the A* handle has %d instances, the planner %d", v.B, h->p.B);
    if (v.H != h->p.G || v.W != h->p.G) return fail(BN_ERR_INVALID, "the A* maps are %d x %d, the planner's grid is %d x %d", v.H, v.W, h->p.G, h->p.G);
    if (h->ad_walk == 1 && !v.jump_current)
        return fail(BN_ERR_STATE, "walk mode 1 needs current jump tables: bn_astar_jump_build_async must follow the A* handle's latest solve");
    BN_BIND(h);
    if (int rc = settle_point(h)) return rc;
    if (int rc = flush_tail(h)) return rc;
    if (int rc = guard_foreign_overlap(h)) return rc;
    const size_t B = h->p.B;
    if (!h->d_ad_i)
        if (int rc = astar_dwa_clear(h)) return rc;
    bn::EpisodeLog &lg = h->ad_log;
    if (int rc = lg.reserve(h->ad_bufs, h->stream, n_steps, table_fail)) return rc;
    const hipMemcpyKind kind = where == BN_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    BN_HIP(hipMemcpyAsync(h->d_ad_state, states0, B * 3 * sizeof(float), kind, h->stream));
    if (where == BN_MEM_HOST) BN_HIP(hipStreamSynchronize(h->stream));   // (pageable source: one upload, before the loop)
    BN_HIP(hipStreamWaitEvent(h->stream, v.solved, 0));                 // behind a's latest solve, without the host
    if (h->ad_walk == 1) BN_HIP(hipStreamWaitEvent(h->stream, v.jump_built, 0));   // ... and its table build
    const AdWords w = ad_words(h);
    bn::AstarDwaArgs x{};
    x.next = v.next; x.arisk = v.risk; x.ainst = v.inst; x.aerr = v.err; x.H = v.H; x.W = v.W;
    if (h->ad_walk == 1) { x.hops = v.hops; x.jump = v.jump; x.jerr = v.jerr; x.levels = v.levels; }
    x.state = h->d_ad_state; x.prev = prev_action_device;
    x.root = w.root(); x.status = w.status(); x.status_step = w.status_step(); x.done = w.done(); x.err = w.err();
    x.log = lg.columns(); x.log_subgoal = lg.extra(0);
    x.z = z_device;
    x.alim0 = a_lim[0]; x.alim1 = a_lim[1]; x.dwa_dt = dwa_delta_t; x.lookahead = lookahead;
    x.nv = num_lin_vel; x.nw = num_ang_vel;
    x.step0 = h->ad_step;
    // chained launches on one stream.  A step walks the path twice at most (2 H W hops): the node budget keeps one launch short
    // on large maps with long paths (64^2: 256 steps, 256^2: 16, 512^2: 4)
    const int per_launch = (int)std::max<int64_t>(1, std::min<int64_t>(bn::kAstarDwaStepsPerLaunch,
                                                                          bn::kAstarDwaNodesPerLaunch / ((int64_t)v.H * v.W)));
    for (int s0 = 0; s0 < n_steps; s0 += per_launch) {
        x.s0 = s0;
        x.ns = std::min(per_launch, n_steps - s0);
        BN_HIP(bn::launch_astar_dwa(h->p, x, h->stream));
    }
    if (bn::astar_add_reader(a, h->stream) != BN_OK) return fail(BN_ERR_HIP, "%s", bn_astar_last_error());
    h->ad_step += (uint64_t)n_steps;
    lg.len = n_steps;
    return BN_OK;
}

int bn_astar_dwa_episode_log(bn_mppi_t *h, float *states, float *rewards, float *actions, float *sub_goals,
                             int32_t *done_step, int32_t *status, int32_t *status_step)
{
    if (!h) return fail(BN_ERR_INVALID, "null handle");
    const bn::EpisodeLog &lg = h->ad_log;
    if (lg.empty()) return fail(BN_ERR_STATE, "no A* + DWA episode has been run");
    BN_BIND(h);
    if (int rc = settle_point(h)) return rc;
    BN_HIP(hipStreamSynchronize(h->stream));
    const size_t B = h->p.B;
    const AdWords w = ad_words(h);
    if (int rc = lg.copy_out(states, rewards, actions, table_fail)) return rc;
    if (sub_goals) BN_HIP(hipMemcpy(sub_goals, lg.extra(0), lg.rows() * 2 * sizeof(float), hipMemcpyDeviceToHost));
    if (status) BN_HIP(hipMemcpy(status, w.status(), B * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (status_step) BN_HIP(hipMemcpy(status_step, w.status_step(), B * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (done_step) BN_HIP(hipMemcpy(done_step, w.done(), B * sizeof(int32_t), hipMemcpyDeviceToHost));
    int32_t err = 0;
    BN_HIP(hipMemcpy(&err, w.err(), sizeof(int32_t), hipMemcpyDeviceToHost));
    if (err) return fail(BN_ERR_STATE, "a next-hop walk broke (more than H*W nodes, or onto an unreachable cell): the A* field is not a valid solve");
    return BN_OK;
}

int bn_astar_dwa_episode_buffers(bn_mppi_t *h, const float **states_device, const float **rewards_device,
                                 const int32_t **done_step_device, const int32_t **status_device, int32_t *n_steps, int32_t *row_capacity)
{
    if (!h) return fail(BN_ERR_INVALID, "null handle");
    const bn::EpisodeLog &lg = h->ad_log;
    if (lg.empty()) return fail(BN_ERR_STATE, "no A* + DWA episode has been run");
    BN_BIND(h);
    if (int rc = settle_point(h)) return rc;
    if (states_device) *states_device = lg.states();                                           // (row_capacity + 1, B, 3)
    if (rewards_device) *rewards_device = lg.reward();                                         // (row_capacity, B)
    if (done_step_device) *done_step_device = ad_words(h).done();                              // (B)
    if (status_device) *status_device = ad_words(h).status();                                  // (B) bn_astar_dwa_status
    if (n_steps) *n_steps = lg.len;
    if (row_capacity) *row_capacity = lg.cap;
    return BN_OK;
}

// ---- the CL-RRT plan-follow-replan loop (clrrt_loop.hip) ----

// what bn_clrrt_loop_reset verified once: the CL-RRT handle plans on the environment's grid
static int clrrt_loop_view(bn_mppi *h, bn_clrrt_t *c, bn::ClrrtView *v)
{
    if (bn::clrrt_view(c, v) != BN_OK) return fail(BN_ERR_INVALID, "%s", bn_clrrt_last_error());
    const bn_clrrt_config &k = v->cfg;
    const bn::SolveParams &p = h->p;
    if (v->device != h->cfg.device_id) return fail(BN_ERR_INVALID, "the CL-RRT handle is on device %d, the environment on device %d", v->device, h->cfg.device_id);
    if (v->B != p.B) return fail(BN_ERR_INVALID, "the CL-RRT handle has %d instances, the environment %d", v->B, p.B);
    if (k.grid_size != p.G || (float)k.resolution != p.res) return fail(BN_ERR_INVALID, "the CL-RRT handle's grid (%d cells of %g) is not the environment's (%d of %g)", k.grid_size, k.resolution, p.G, (double)p.res);
    if ((float)k.x_limits[0] != p.x0 || (float)k.x_limits[1] != p.x_hi || (float)k.y_limits[0] != p.y0 || (float)k.y_limits[1] != p.y_hi)
        return fail(BN_ERR_INVALID, "the CL-RRT handle's limits are not the environment's");
    if ((float)k.u_min[0] != p.umin0 || (float)k.u_min[1] != p.umin1 || (float)k.u_max[0] != p.umax0 || (float)k.u_max[1] != p.umax1)
        return fail(BN_ERR_INVALID, "the CL-RRT handle's action bounds are not the environment's");
    if (!v->have_map) return fail(BN_ERR_STATE, "bn_clrrt_set_map must precede the loop");
    return BN_OK;
}

int bn_clrrt_loop_reset(bn_mppi_t *h, bn_clrrt_t *c, const float *goal_nodes, const uint64_t *seeds, double delta_t, double time_limit)
{
    if (!h || !c || !goal_nodes || !seeds) return fail(BN_ERR_INVALID, "null argument");
    if (!std::isfinite(time_limit)) return fail(BN_ERR_INVALID, "time_limit must be finite");
    if (!h->env_attached) return fail(BN_ERR_STATE, "bn_mppi_env_attach must precede bn_clrrt_loop_reset");
    if ((float)delta_t != h->p.env_dt) return fail(BN_ERR_INVALID, "delta_t (%g) is not the environment's (%g)", delta_t, (double)h->p.env_dt);
    bn::ClrrtView v;
    if (int rc = clrrt_loop_view(h, c, &v)) return rc;
    BN_BIND(h);
    if (int rc = settle_point(h)) return rc;
    if (int rc = flush_tail(h)) return rc;
    const size_t B = h->p.B;
    if (h->cl_bufs.list.empty()) {
        h->cl_bufs.add(&h->d_cl_rover, B * sizeof(bn::ClrrtRover));
        h->cl_bufs.add(&h->d_cl_flags, ClFlags::count(B) * sizeof(int32_t));
        h->cl_bufs.add(&h->d_cl_goal, B * 3 * sizeof(float));
        h->cl_bufs.add(&h->d_cl_words, bn::ClrrtOutcome::count(B) * sizeof(int32_t));
        h->cl_bufs.add_pinned(&h->h_cl_pending, sizeof(int32_t));
        h->cl_bufs.add_event(&h->cl_ev[0]);
        h->cl_bufs.add_event(&h->cl_ev[1]);
        h->cl_log.attach(h->cl_bufs, B, 3);            // + deviation, plan index, event; grows with the longest run
    }
    if (int rc = h->cl_bufs.ensure(table_fail)) return rc;
    BN_HIP(hipStreamSynchronize(h->stream));                               // a previous episode's launches are done with the words below
    std::vector<bn::ClrrtRover> r0(B, bn::ClrrtRover{0, BN_CL_RUNNING, 1, 0, 0, 0, 0, -1});
    BN_HIP(hipMemcpy(h->d_cl_rover, r0.data(), B * sizeof(bn::ClrrtRover), hipMemcpyHostToDevice));
    BN_HIP(hipMemset(h->d_cl_flags, 0, ClFlags::count(B) * sizeof(int32_t)));
    BN_HIP(hipMemcpy(h->d_cl_goal, goal_nodes, B * 3 * sizeof(float), hipMemcpyHostToDevice));
    if (bn::clrrt_loop_reset(c, h->stream, goal_nodes, seeds) != BN_OK) return fail(BN_ERR_INVALID, "%s", bn_clrrt_last_error());
    // PlanetaryEnv: elapsed += delta_t in float64, elapsed > time_limit after the step: the first step count at which that holds
    double elapsed = 0.0;
    int32_t k = 0;
    const double dt = delta_t;                     // the Python float, not its float32 rounding: 5 x 0.1 is exactly 0.5, 5 x 0.1f is above it
    if (dt > 0.0) {
        while (!(elapsed > time_limit) && k < INT32_MAX) { elapsed += dt; ++k; }
    } else {
        k = INT32_MAX;
    }
    h->cl_limit_steps = k;
    h->cl_iter = 0;
    h->cl_log.len = 0;
    h->cl_ready = true;
    h->cl_planner = c;
    return BN_OK;
}

int bn_clrrt_loop_run(bn_mppi_t *h, bn_clrrt_t *c, int32_t n, float *states_device, const float *z_device,
                      const float *samples_device, int32_t num_tables, uint32_t flags, float *follow_ms)
{
    if (!h || !c || !states_device) return fail(BN_ERR_INVALID, "null argument");
    if (n < 1 || n > (1 << 24)) return fail(BN_ERR_INVALID, "n must be in [1, 2^24]");
    if (num_tables < 0) return fail(BN_ERR_INVALID, "num_tables must be >= 0");
    if (!h->cl_ready) return fail(BN_ERR_STATE, "bn_clrrt_loop_reset must precede bn_clrrt_loop_run");
    if (c != h->cl_planner) return fail(BN_ERR_INVALID, "this is not the CL-RRT handle bn_clrrt_loop_reset was given: the episode's goals, streams and plans live in that one");
    if (!h->env_attached || !h->goal_set) return fail(BN_ERR_STATE, "bn_mppi_env_attach and the goals must precede bn_clrrt_loop_run");
    if ((int64_t)h->cl_iter + n > INT32_MAX) return fail(BN_ERR_INVALID, "the episode's iteration count exceeds 2^31 - 1");
    bn::ClrrtView v;
    if (int rc = clrrt_loop_view(h, c, &v)) return rc;
    BN_BIND(h);
    if (int rc = settle_point(h)) return rc;
    if (int rc = flush_tail(h)) return rc;
    if (int rc = guard_foreign_overlap(h)) return rc;
    bn::EpisodeLog &lg = h->cl_log;
    if (int rc = lg.reserve(h->cl_bufs, h->stream, n, table_fail)) return rc;
    const ClFlags f = cl_flags(h);
    bn::ClrrtFollowArgs x{};
    x.rover = h->d_cl_rover; x.state = states_device; x.starts = v.starts; x.goal_nodes = h->d_cl_goal;
    x.path_actions = v.path_actions; x.path_states = v.path_states; x.results = v.results;
    x.active = f.active(); x.pending = f.pending(); x.psamples = v.samples;
    x.inj = samples_device; x.P = samples_device ? num_tables : 0; x.iters = v.iters; x.path_cap = v.path_cap;
    x.log = lg.columns(); x.log_dev = lg.extra(0);
    x.log_plan = reinterpret_cast<int32_t *>(lg.extra(1)); x.log_event = reinterpret_cast<int32_t *>(lg.extra(2));
    x.z = z_device; x.iter0 = h->cl_iter; x.n = n; x.limit_steps = h->cl_limit_steps; x.use_lds = (flags & 1u) ? 0 : 1;
    x.xlo = v.cfg.x_limits[0]; x.xhi = v.cfg.x_limits[1]; x.ylo = v.cfg.y_limits[0]; x.yhi = v.cfg.y_limits[1];
    float ms_total = 0.0f;
    // One host round trip per ROUND of replans: every pending rover takes its plan and at least one iteration (or a status) in the
    // next follow launch, so n + 2 rounds bound the loop.
    for (int64_t round = 0; round < (int64_t)n + 2; ++round) {
        if (follow_ms) BN_HIP(hipEventRecord(h->cl_ev[0], h->stream));
        BN_HIP(bn::launch_clrrt_follow(h->p, x, h->stream));
        if (follow_ms) BN_HIP(hipEventRecord(h->cl_ev[1], h->stream));
        BN_HIP(hipMemcpyAsync(h->h_cl_pending, f.pending(), sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        BN_HIP(hipStreamSynchronize(h->stream));
        if (follow_ms) {
            float ms = 0.0f;
            BN_HIP(hipEventElapsedTime(&ms, h->cl_ev[0], h->cl_ev[1]));
            ms_total += ms;
        }
        if (*h->h_cl_pending == 0) break;
        if (bn::clrrt_plan_masked(c, h->stream, f.active(), samples_device ? 0 : 1) != BN_OK) return fail(BN_ERR_HIP, "%s", bn_clrrt_last_error());
        BN_HIP(hipMemsetAsync(f.pending(), 0, sizeof(int32_t), h->stream));     // (the follow kernel clears the mask words it takes)
    }
    BN_HIP(bn::launch_clrrt_outcome(h->d_cl_rover, bn::ClrrtOutcome{h->d_cl_words, (size_t)h->p.B}, h->stream));
    if (follow_ms) *follow_ms = ms_total;
    h->cl_iter += n;
    lg.len = n;
    return BN_OK;
}

int bn_clrrt_loop_log(bn_mppi_t *h, float *states, float *rewards, float *actions, float *deviations, int32_t *plan_index,
                      int32_t *events, int32_t *done_iter, int32_t *status, int32_t *plans, int32_t *steps)
{
    if (!h) return fail(BN_ERR_INVALID, "null handle");
    const bn::EpisodeLog &lg = h->cl_log;
    if (lg.empty()) return fail(BN_ERR_STATE, "no CL-RRT loop has been run");
    BN_BIND(h);
    if (int rc = settle_point(h)) return rc;
    BN_HIP(hipStreamSynchronize(h->stream));
    const size_t B = h->p.B;
    if (int rc = lg.copy_out(states, rewards, actions, table_fail)) return rc;
    if (deviations) BN_HIP(hipMemcpy(deviations, lg.extra(0), lg.rows() * sizeof(float), hipMemcpyDeviceToHost));
    if (plan_index) BN_HIP(hipMemcpy(plan_index, lg.extra(1), lg.rows() * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (events) BN_HIP(hipMemcpy(events, lg.extra(2), lg.rows() * sizeof(int32_t), hipMemcpyDeviceToHost));
    std::vector<bn::ClrrtRover> r(B);
    BN_HIP(hipMemcpy(r.data(), h->d_cl_rover, B * sizeof(bn::ClrrtRover), hipMemcpyDeviceToHost));
    for (size_t b = 0; b < B; ++b) {
        if (done_iter) done_iter[b] = r[b].done_iter;
        if (status) status[b] = r[b].status;
        if (plans) plans[b] = r[b].plans;
        if (steps) steps[b] = r[b].steps;
    }
    return BN_OK;
}

int bn_clrrt_loop_episode_buffers(bn_mppi_t *h, const float **states_device, const float **rewards_device,
                                  const int32_t **done_step_device, const int32_t **stopped_device, int32_t *n_iterations, int32_t *row_capacity)
{
    if (!h) return fail(BN_ERR_INVALID, "null handle");
    const bn::EpisodeLog &lg = h->cl_log;
    if (lg.empty()) return fail(BN_ERR_STATE, "no CL-RRT loop has been run");
    BN_BIND(h);
    if (int rc = settle_point(h)) return rc;
    const bn::ClrrtOutcome w{h->d_cl_words, (size_t)h->p.B};
    if (states_device) *states_device = lg.states();                                           // (row_capacity + 1, B, 3)
    if (rewards_device) *rewards_device = lg.reward();                                         // (row_capacity, B)
    if (done_step_device) *done_step_device = w.done_step();                                   // (B)
    if (stopped_device) *stopped_device = w.stopped();                                         // (B)
    if (n_iterations) *n_iterations = lg.len;
    if (row_capacity) *row_capacity = lg.cap;
    return BN_OK;
}

int bn_clrrt_loop_rover_buffers(bn_mppi_t *h, const int32_t **status_device, const int32_t **plans_device)
{
    if (!h) return fail(BN_ERR_INVALID, "null handle");
    if (h->cl_log.empty()) return fail(BN_ERR_STATE, "no CL-RRT loop has been run");
    const bn::ClrrtOutcome w{h->d_cl_words, (size_t)h->p.B};
    if (status_device) *status_device = w.status();
    if (plans_device) *plans_device = w.plans();
    return BN_OK;
}

int bn_clrrt_loop_set_plans(bn_mppi_t *h, bn_clrrt_t *c, const float *actions, const float *states, const int32_t *lengths,
                            int32_t max_length, int32_t iteration)
{
    if (!h || !c || !actions || !states || !lengths) return fail(BN_ERR_INVALID, "null argument");
    if (!h->cl_ready) return fail(BN_ERR_STATE, "bn_clrrt_loop_reset must precede bn_clrrt_loop_set_plans");
    if (c != h->cl_planner) return fail(BN_ERR_INVALID, "this is not the CL-RRT handle bn_clrrt_loop_reset was given: the episode's goals, streams and plans live in that one");
    bn::ClrrtView v;
    if (int rc = clrrt_loop_view(h, c, &v)) return rc;
    if (max_length < 1 || max_length > v.path_cap) return fail(BN_ERR_INVALID, "max_length must be in [1, path_cap = %d]", v.path_cap);
    const size_t B = h->p.B, Lm = (size_t)max_length;
    for (size_t b = 0; b < B; ++b)
        if (lengths[b] < 1 || lengths[b] > max_length) return fail(BN_ERR_INVALID, "lengths must be in [1, max_length]");
    BN_BIND(h);
    if (int rc = settle_point(h)) return rc;
    BN_HIP(hipStreamSynchronize(h->stream));
    std::vector<bn::ClrrtRover> r(B);
    BN_HIP(hipMemcpy(r.data(), h->d_cl_rover, B * sizeof(bn::ClrrtRover), hipMemcpyDeviceToHost));
    for (size_t b = 0; b < B; ++b) {
        BN_HIP(hipMemcpy(v.path_actions + b * (size_t)v.path_cap * 2, actions + b * Lm * 2, (size_t)lengths[b] * 2 * sizeof(float), hipMemcpyHostToDevice));
        BN_HIP(hipMemcpy(v.path_states + b * ((size_t)v.path_cap + 1) * 3, states + b * (Lm + 1) * 3, ((size_t)lengths[b] + 1) * 3 * sizeof(float), hipMemcpyHostToDevice));
        r[b].need = 0; r[b].aidx = 0; r[b].length = lengths[b];
        if (iteration >= 0) r[b].iter = iteration;
    }
    BN_HIP(hipMemcpy(h->d_cl_rover, r.data(), B * sizeof(bn::ClrrtRover), hipMemcpyHostToDevice));
    BN_HIP(hipMemset(h->d_cl_flags, 0, ClFlags::count(B) * sizeof(int32_t)));
    if (iteration >= 0) h->cl_iter = iteration;
    return BN_OK;
}

}  // extern "C"
