// mppi_env.cpp -- the device-side closed loop of the C ABI: the environment (bn_mppi_env_*), the fused episode
// (bn_mppi_episode_async: a batch of solves whose launches advance the state themselves) and the DWA entry points.
#include "mppi_handle.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

using namespace bn::host;

namespace {

// The scratch block of the DWA entry points, in floats: actions | stage goal | X | cost | w | best | best states | states.
// The one place the layout is written: bn_mppi_dwa_solve and bn_mppi_dwa_forward_async fill it, bn_mppi_dwa_buffers and
// bn_mppi_dwa_candidates hand out views of it.
struct DwaScratch {
    size_t n_act, n_goal, n_X, n_c, n_bs, floats;
    size_t B;
    DwaScratch(size_t B_, size_t NA, size_t T)
        : n_act(B_ * NA * 2), n_goal(B_ * 2), n_X(B_ * NA * (T + 1) * 3), n_c(B_ * NA), n_bs(B_ * (T + 1) * 3),
          floats(n_act + n_goal + n_X + 2 * n_c + B_ + n_bs + B_ * 3), B(B_) {}
    float *actions(float *s) const { return s; }                                   // (B, num_actions, 2)
    float *stage_goal(float *s) const { return s + n_act; }                        // (B, 2)
    float *X(float *s) const { return stage_goal(s) + n_goal; }                    // (B, num_actions, T + 1, 3)
    float *cost(float *s) const { return X(s) + n_X; }                             // (B, num_actions)
    float *w(float *s) const { return cost(s) + n_c; }                             // (B, num_actions)
    int *best(float *s) const { return reinterpret_cast<int *>(w(s) + n_c); }      // (B)
    float *best_states(float *s) const { return w(s) + n_c + B; }                  // (B, T + 1, 3)
    float *states(float *s) const { return best_states(s) + n_bs; }                // (B, 3)
};

}  // namespace

namespace bn {
namespace host {

void env_release(bn_mppi *h)
{
    h->env_bufs.free_all();
}

}  // namespace host
}  // namespace bn

extern "C" {

int bn_mppi_env_attach(bn_mppi_t *h, const float *latent_mean, const float *latent_std, bn_mem_kind where,
                       float goal_threshold, float delta_t, uint64_t seed)
{
    if (!h || !latent_mean || !latent_std) return fail(BN_ERR_INVALID, "null argument");
    if (!(goal_threshold >= 0.0f) || !(delta_t > 0.0f)) return fail(BN_ERR_INVALID, "goal_threshold >= 0 and delta_t > 0 required");
    BN_BIND(h);
    if (int rc = settle_point(h)) return rc;
    if (int rc = flush_tail(h)) return rc;
    BN_HIP(hipStreamSynchronize(h->stream));
    const size_t bytes = (size_t)h->n_maps * h->p.G * h->p.G * 4;
    if (h->env_bufs.list.empty()) {                    // the environment's group, built by the first attach; the episode log grows on demand
        h->env_bufs.add(&h->d_lat_mean, bytes);
        h->env_bufs.add(&h->d_lat_std, bytes);
        h->env_bufs.add(&h->d_env_state, (size_t)h->p.B * 3 * 4);
        h->env_bufs.add(&h->d_ep_done, (size_t)h->p.B * sizeof(int));
        h->ep_log.attach(h->env_bufs, h->p.B, 0);
    }
    if (!h->env_bufs.live) {
        if (int rc = h->env_bufs.ensure(table_fail)) return rc;
        if (int rc = fills_done()) return rc;
    }
    const hipMemcpyKind kind = where == BN_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    BN_HIP(hipMemcpy(h->d_lat_mean, latent_mean, bytes, kind));
    BN_HIP(hipMemcpy(h->d_lat_std, latent_std, bytes, kind));
    h->p.lat_mean = h->d_lat_mean; h->p.lat_std = h->d_lat_std; h->p.env_state = h->d_env_state; h->p.ep_done = h->d_ep_done;
    h->p.goal_thr = goal_threshold; h->p.env_dt = delta_t; h->p.env_seed = seed;
    // latency kernel, overlapped episodes: how far one environment step can move the start cell (see SolveParams::spec_extra)
    h->p.spec_extra = 0;
    if (h->lat_kernel && h->d_gran[0] && !exp_env("BN_NO_SPEC_WINDOW")) {
        const double vmax = std::max(std::fabs((double)h->p.umin0), std::fabs((double)h->p.umax0));
        const double cells = std::floor(vmax * (double)delta_t / (double)h->p.res) + 1.0;
        if (cells <= 8.0 && h->p.WN + 2 * (int)cells <= h->p.G + 1) {
            h->p.spec_extra = (int)cells;
            if (bn::lat_lds_bytes(h->p) == 0) h->p.spec_extra = 0;      // would not fit the LDS
        }
    }
    h->env_attached = true;
    return BN_OK;
}

int bn_mppi_env_set_freeze(bn_mppi_t *h, int32_t freeze_on_goal)
{
    if (!h) return fail(BN_ERR_INVALID, "null handle");
    BN_BIND(h);
    if (int rc = settle_point(h)) return rc;
    if (int rc = flush_tail(h)) return rc;
    h->p.env_freeze = freeze_on_goal ? 1 : 0;
    return BN_OK;
}

int bn_mppi_env_step(bn_mppi_t *h, const float *actions_device, float *states_device, float *rewards_device,
                     int32_t *terminated_device, const float *z_device, uint64_t step_index)
{
    if (!h || !actions_device || !states_device || !rewards_device || !terminated_device) return fail(BN_ERR_INVALID, "null argument");
    if (!h->env_attached) return fail(BN_ERR_STATE, "bn_mppi_env_attach must precede bn_mppi_env_step");
    BN_BIND(h);
    if (int rc = settle_point(h)) return rc;
    if (int rc = guard_foreign_overlap(h)) return rc;
    BN_HIP(bn::launch_env_step(h->p, actions_device, states_device, rewards_device, terminated_device, z_device, step_index, h->stream));
    return BN_OK;
}

int bn_mppi_env_collision_check(bn_mppi_t *h, const float *states_device, int32_t n_positions, float stuck_threshold,
                                const float *z_device, uint64_t draw_index, uint8_t *out_device)
{
    if (!h || !states_device || !out_device) return fail(BN_ERR_INVALID, "null argument");
    if (n_positions < 1) return fail(BN_ERR_INVALID, "n_positions must be >= 1");
    if (!h->env_attached) return fail(BN_ERR_STATE, "bn_mppi_env_attach must precede bn_mppi_env_collision_check");
    BN_BIND(h);
    if (int rc = settle_point(h)) return rc;
    if (int rc = guard_foreign_overlap(h)) return rc;
    BN_HIP(bn::launch_env_collision(h->p, states_device, n_positions, stuck_threshold, z_device, draw_index, out_device, h->stream));
    return BN_OK;
}

int bn_mppi_episode_async(bn_mppi_t *h, int32_t n_steps, const float *states0, bn_mem_kind states_where, const float *eps,
                          bn_noise_kind noise, int32_t eps_ring, int64_t eps_stride, const float *z_device)
{
    if (!h) return fail(BN_ERR_INVALID, "null handle");
    if (!h->env_attached) return fail(BN_ERR_STATE, "bn_mppi_env_attach must precede bn_mppi_episode_async");
    if (h->slow_path) return fail(BN_ERR_INVALID, "the fused device-side closed loop is not available on the slow path (a horizon beyond the role kernels' LDS, or the "
                                                   "reference-order arithmetic together with sampled slip): drive bn_mppi_forward_async + bn_mppi_env_step instead");
    if (!h->pipelined) return fail(BN_ERR_INVALID, "the device-side closed loop needs the pipelined mode (num_samples <= 4096)");
    if (n_steps < 1) return fail(BN_ERR_INVALID, "n_steps must be >= 1");
    BN_BIND(h);
    if (int rc = flush_tail(h)) return rc;            // anything pending belongs to the pre-episode state
    const size_t B = h->p.B;
    bn::EpisodeLog &lg = h->ep_log;
    if (int rc = lg.reserve(h->env_bufs, h->stream, n_steps, table_fail)) return rc;
    h->p.ep_states = lg.states(); h->p.ep_reward = lg.reward(); h->p.ep_action = lg.action();
    BN_HIP(hipMemsetAsync(h->d_ep_done, 0xff, B * sizeof(int), h->stream));        // -1: goal not reached
    if (!states0) return fail(BN_ERR_INVALID, "states0 is null");
    if (states_where == BN_MEM_HOST) {                 // one upload; the loop below must not touch the host again
        BN_HIP(hipStreamSynchronize(h->stream));
        BN_HIP(hipMemcpy(h->d_state, states0, B * 3 * 4, hipMemcpyHostToDevice));
        states0 = h->d_state;
        states_where = BN_MEM_DEVICE;
    }
    journal_arm_states(h);                            // the first step's launch keeps states0 for a re-run
    h->in_episode = true;
    lg.len = 0;                                       // every enqueued solve counts itself in (mppi_solve.cpp)
    h->ep_z = z_device;
    int rc = bn_mppi_solve_n_async(h, n_steps, states0, states_where, eps, noise, eps_ring, eps_stride);
    if (rc == BN_OK) rc = flush_tail(h);              // the last solve's tail and the last environment step
    h->in_episode = false;
    if (rc == BN_OK) journal_push(h, bn_mppi::BatchRec{n_steps, states0, eps, noise, eps_ring, eps_stride, true, z_device}, noise != BN_NOISE_HOST_KT2);
    return rc;
}

int bn_mppi_episode_log(bn_mppi_t *h, float *states_host, float *rewards_host, float *actions_host, int32_t *done_step_host)
{
    if (!h) return fail(BN_ERR_INVALID, "null handle");
    if (h->ep_log.empty()) return fail(BN_ERR_STATE, "no episode has been run");
    BN_BIND(h);
    if (int rc = settle_point(h)) return rc;
    BN_HIP(hipStreamSynchronize(h->stream));
    if (int rc = h->ep_log.copy_out(states_host, rewards_host, actions_host, table_fail)) return rc;
    if (done_step_host) BN_HIP(hipMemcpy(done_step_host, h->d_ep_done, (size_t)h->p.B * sizeof(int), hipMemcpyDeviceToHost));
    return BN_OK;
}

int bn_mppi_episode_buffers(bn_mppi_t *h, const float **states_device, const float **rewards_device, const int32_t **done_step_device,
                            int32_t *n_steps, int32_t *row_capacity)
{
    if (!h) return fail(BN_ERR_INVALID, "null handle");
    const bn::EpisodeLog &lg = h->ep_log;
    if (lg.empty()) return fail(BN_ERR_STATE, "no episode has been run");
    BN_BIND(h);
    if (int rc = settle_point(h)) return rc;              // from here on the episode is ordered on the handle's stream
    if (states_device) *states_device = lg.states();                                           // (row_capacity + 1, B, 3)
    if (rewards_device) *rewards_device = lg.reward();                                         // (row_capacity, B)
    if (done_step_device) *done_step_device = h->d_ep_done;                                    // (B)
    if (n_steps) *n_steps = lg.len;
    if (row_capacity) *row_capacity = lg.cap;
    return BN_OK;
}

int bn_mppi_dwa_solve(bn_mppi_t *h, const float *states_host, const float *actions_host, int32_t num_actions,
                      const float *stage_goal_host, float *best_action_host, float *best_states_host,
                      float *costs_host, float *weights_host, float *states_all_host, int32_t *best_index_host)
{
    if (!h || !states_host || !actions_host) return fail(BN_ERR_INVALID, "null argument");
    if (num_actions < 1 || num_actions > 1024) return fail(BN_ERR_INVALID, "num_actions must be in [1, 1024]");
    if (!h->map_set || !h->goal_set) return fail(BN_ERR_STATE, "set_map and set_goal must precede dwa_solve");
    BN_BIND(h);
    if (int rc = settle_point(h)) return rc;
    if (int rc = flush_tail(h)) return rc;
    const size_t B = h->p.B, NA = num_actions;
    const DwaScratch s(B, NA, h->p.T);
    const size_t n_act = s.n_act, n_goal = s.n_goal, n_X = s.n_X, n_c = s.n_c, n_bs = s.n_bs;
    if (int rc = ensure_scratch(h, s.floats * 4)) return rc;
    float *d_act = s.actions(h->d_scratch), *d_goal = s.stage_goal(h->d_scratch), *d_X = s.X(h->d_scratch), *d_c = s.cost(h->d_scratch), *d_w = s.w(h->d_scratch);
    int *d_best = s.best(h->d_scratch);
    float *d_bs = s.best_states(h->d_scratch), *d_st = s.states(h->d_scratch);
    // one staged upload (actions | stage goal) + the states, one launch, the downloads queued behind it, one wait
    h->dwa_stage.resize(n_act + n_goal);
    std::memcpy(h->dwa_stage.data(), actions_host, n_act * 4);
    if (stage_goal_host) std::memcpy(h->dwa_stage.data() + n_act, stage_goal_host, n_goal * 4);
    BN_HIP(hipStreamSynchronize(h->stream));            // the staging vector and the scratch may still feed a previous call
    BN_HIP(hipMemcpyAsync(d_act, h->dwa_stage.data(), (n_act + (stage_goal_host ? n_goal : 0)) * 4, hipMemcpyHostToDevice, h->stream));
    if (!stage_goal_host) BN_HIP(hipMemcpyAsync(d_goal, h->d_goal, n_goal * 4, hipMemcpyDeviceToDevice, h->stream));   // no reference path: the goal (dwa.py:243-247)
    BN_HIP(hipMemcpyAsync(d_st, states_host, B * 3 * 4, hipMemcpyHostToDevice, h->stream));
    bn::SolveParams p = h->p;
    p.state = d_st;
    BN_HIP(bn::launch_dwa(p, d_act, d_goal, num_actions, d_X, d_c, d_w, d_best, d_bs, nullptr, h->stream));
    std::vector<int> best(B);
    BN_HIP(hipMemcpyAsync(best.data(), d_best, B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (best_states_host) BN_HIP(hipMemcpyAsync(best_states_host, d_bs, n_bs * 4, hipMemcpyDeviceToHost, h->stream));
    if (costs_host) BN_HIP(hipMemcpyAsync(costs_host, d_c, n_c * 4, hipMemcpyDeviceToHost, h->stream));
    if (weights_host) BN_HIP(hipMemcpyAsync(weights_host, d_w, n_c * 4, hipMemcpyDeviceToHost, h->stream));
    if (states_all_host) BN_HIP(hipMemcpyAsync(states_all_host, d_X, n_X * 4, hipMemcpyDeviceToHost, h->stream));
    BN_HIP(hipStreamSynchronize(h->stream));
    for (size_t b = 0; b < B; ++b) {
        if (best_index_host) best_index_host[b] = best[b];
        if (best_action_host) std::memcpy(best_action_host + b * 2, actions_host + (b * NA + best[b]) * 2, 8);
    }
    return BN_OK;
}

int bn_mppi_dwa_forward_async(bn_mppi_t *h, const float *states_device, float *prev_action_device, const float a_lim_host[2],
                              float dwa_delta_t, int32_t num_lin_vel, int32_t num_ang_vel, const float *path_device, int32_t num_path,
                              float lookahead, float *best_states_device)
{
    if (!h || !states_device || !prev_action_device || !a_lim_host) return fail(BN_ERR_INVALID, "null argument");
    const int64_t NA = (int64_t)num_lin_vel * num_ang_vel;
    if (num_lin_vel < 1 || num_ang_vel < 1 || NA > 1024) return fail(BN_ERR_INVALID, "num_lin_vel * num_ang_vel must be in [1, 1024]");
    if (path_device && num_path < 1) return fail(BN_ERR_INVALID, "a reference path needs at least one point");
    if (!h->map_set || !h->goal_set) return fail(BN_ERR_STATE, "set_map and set_goal must precede dwa_forward");
    BN_BIND(h);
    if (int rc = settle_point(h)) return rc;
    if (int rc = flush_tail(h)) return rc;
    const DwaScratch s(h->p.B, (size_t)NA, h->p.T);
    if (s.floats * 4 > h->scratch_bytes) BN_HIP(hipStreamSynchronize(h->stream));      // growing frees the old block: nothing may still use it
    if (int rc = ensure_scratch(h, s.floats * 4)) return rc;
    float *d_act = s.actions(h->d_scratch), *d_goal = s.stage_goal(h->d_scratch), *d_X = s.X(h->d_scratch), *d_c = s.cost(h->d_scratch), *d_w = s.w(h->d_scratch);
    int *d_best = s.best(h->d_scratch);
    float *d_bs = best_states_device ? best_states_device : s.best_states(h->d_scratch);
    bn::SolveParams p = h->p;
    p.state = states_device;
    BN_HIP(bn::launch_dwa_window(p, prev_action_device, a_lim_host, dwa_delta_t, num_lin_vel, num_ang_vel, path_device, num_path, lookahead,
                                 d_act, d_goal, h->stream));
    BN_HIP(bn::launch_dwa(p, d_act, d_goal, (int)NA, d_X, d_c, d_w, d_best, d_bs, prev_action_device, h->stream));
    return BN_OK;
}

int bn_mppi_dwa_buffers(bn_mppi_t *h, int32_t num_actions, const float **states_all_device, const float **costs_device,
                        const float **weights_device)
{
    if (!h) return fail(BN_ERR_INVALID, "null handle");
    if (num_actions < 1 || num_actions > 1024) return fail(BN_ERR_INVALID, "num_actions must be in [1, 1024]");
    const DwaScratch s(h->p.B, num_actions, h->p.T);
    if (!h->d_scratch || h->scratch_bytes < s.floats * 4)
        return fail(BN_ERR_STATE, "no bn_mppi_dwa_solve with this num_actions has run");
    if (states_all_device) *states_all_device = s.X(h->d_scratch);
    if (costs_device) *costs_device = s.cost(h->d_scratch);
    if (weights_device) *weights_device = s.w(h->d_scratch);
    return BN_OK;
}

int bn_mppi_dwa_candidates(bn_mppi_t *h, int32_t num_actions, const float **actions_device, const float **stage_goal_device)
{
    if (!h) return fail(BN_ERR_INVALID, "null handle");
    if (num_actions < 1 || num_actions > 1024) return fail(BN_ERR_INVALID, "num_actions must be in [1, 1024]");
    if (!h->d_scratch) return fail(BN_ERR_STATE, "no DWA solve has run");
    const DwaScratch s(h->p.B, num_actions, h->p.T);
    if (actions_device) *actions_device = s.actions(h->d_scratch);                                         // (B, num_actions, 2)
    if (stage_goal_device) *stage_goal_device = s.stage_goal(h->d_scratch);                                // (B, 2)
    return BN_OK;
}

}  // extern "C"
