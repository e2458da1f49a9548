// score_kernels.hip -- an episode log reduced to its outcome on the device.
//
// The three closed loops leave the same kind of log: states (n + 1, B, 3), rewards (n, B) and a per-episode word for the goal.
// bn_episode_score turns B such logs into the benchmark's per-episode figures without copying a row to the host.  One lane owns
// one episode and walks its rows in step order; lane b reads element b of every row, so a wave's loads of a row are contiguous.
// The sums are float64 and sequential, exactly the order of tests/benchmark_spec.py: the device's double square root is the
// only operation whose rounding may differ from the host's.
//
// done_step's convention is the one the loops write (mppi_tail.h `p.ep_done[b] = p.ep_index`, astar_dwa.hip `done = (int)ep`):
// the 0-BASED INDEX OF THE STEP whose resulting state first lay within the goal threshold -- reward row done_step, state row
// done_step + 1 -- or -1.  An episode that reached its goal at step k therefore counts k + 1 rows.
#include "../../include/benchnav_mppi.h"
#include "bn_host.h"

#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <string>

namespace bn {
namespace {

constexpr int kScoreThreads = 64;          // one wave per workgroup: B = 65 already runs two workgroups

struct ScoreOut {
    int32_t *outcome, *steps, *stuck_steps;
    double *time, *path_length, *reward_sum, *final_distance;
    float *reward_min;
};

__global__ __launch_bounds__(kScoreThreads) void episode_score_kernel(const float *__restrict__ states, const float *__restrict__ rewards,
                                                                      const float *__restrict__ goals, const int32_t *__restrict__ end_step,
                                                                      const int32_t *__restrict__ done_step, const int32_t *__restrict__ stopped,
                                                                      const uint8_t *__restrict__ invalid, int n, int B, float stuck_thr,
                                                                      double delta_t, ScoreOut o)
{
    const int b = blockIdx.x * kScoreThreads + threadIdx.x;
    if (b >= B) return;
    const int done = done_step[b];
    // rows that count: the caller's end_step, or (null) every row up to and including the step that reached the goal
    int end = end_step ? end_step[b] : (done >= 0 ? done + 1 : n);
    end = end < 0 ? 0 : (end > n ? n : end);
    const size_t row = (size_t)B * 3;
    double px = (double)states[(size_t)b * 3 + 0], py = (double)states[(size_t)b * 3 + 1];
    double time = 0.0, path = 0.0, rsum = 0.0;
    float rmin = NAN;
    int steps = 0, stuck = 0;
    for (int i = 0; i < end; ++i) {
        const float r = rewards[(size_t)i * B + b];
        const float *nx = states + (size_t)(i + 1) * row + (size_t)b * 3;
        const double x = (double)nx[0], y = (double)nx[1];
        if (!(r != r)) {                                // a NaN reward is "no step": the row adds nothing
            const double dx = x - px, dy = y - py;
            path += sqrt(dx * dx + dy * dy);
            time += delta_t;                            // _elapsed_time += delta_t, one rounding per step
            rsum += (double)r;
            rmin = (steps == 0 || r < rmin) ? r : rmin;
            stuck += r <= stuck_thr ? 1 : 0;
            steps += 1;
        }
        px = x; py = y;                                 // ... but its state is still where the rover is
    }
    const double gx = (double)goals[(size_t)b * 2 + 0] - px, gy = (double)goals[(size_t)b * 2 + 1] - py;
    int outcome = BN_OUTCOME_TIME_LIMIT;
    if (invalid && invalid[b]) outcome = BN_OUTCOME_INVALID;
    else if (done >= 0) outcome = BN_OUTCOME_GOAL;
    else if (stopped && stopped[b] != 0) outcome = BN_OUTCOME_STOPPED;
    o.outcome[b] = outcome;
    o.steps[b] = steps;
    o.stuck_steps[b] = stuck;
    o.time[b] = time;
    o.path_length[b] = path;
    o.reward_sum[b] = rsum;
    o.reward_min[b] = rmin;
    o.final_distance[b] = sqrt(gx * gx + gy * gy);
}

thread_local std::string g_score_error;

int score_fail(int code, const std::string &msg)
{
    g_score_error = msg;
    return code;
}

}  // namespace
}  // namespace bn

extern "C" {

const char *bn_score_last_error(void) { return bn::g_score_error.c_str(); }

int bn_episode_score(int32_t device_id, void *stream, const float *states_device, const float *rewards_device, const float *goals_device,
                     const int32_t *end_step_device, const int32_t *done_step_device, const int32_t *stopped_device,
                     const uint8_t *invalid_device, int32_t n_steps, int32_t num_episodes, float stuck_threshold, double delta_t,
                     int32_t *outcome_device, int32_t *steps_device, double *time_device, double *path_length_device,
                     double *reward_sum_device, float *reward_min_device, int32_t *stuck_steps_device, double *final_distance_device)
{
    using bn::score_fail;
    if (!states_device || !rewards_device || !goals_device || !done_step_device) return score_fail(BN_ERR_INVALID, "null argument");
    if (!outcome_device || !steps_device || !time_device || !path_length_device || !reward_sum_device || !reward_min_device ||
        !stuck_steps_device || !final_distance_device)
        return score_fail(BN_ERR_INVALID, "null output");
    if (n_steps < 1) return score_fail(BN_ERR_INVALID, "n_steps must be >= 1");
    if (num_episodes < 1) return score_fail(BN_ERR_INVALID, "num_episodes must be >= 1");
    if (!(delta_t > 0.0)) return score_fail(BN_ERR_INVALID, "delta_t must be > 0");
    if (int rc = bn::open_device(device_id, score_fail)) return rc;
    BN_ON_DEVICE(score_fail, device_id);
    const bn::ScoreOut o{outcome_device, steps_device, stuck_steps_device, time_device, path_length_device, reward_sum_device,
                         final_distance_device, reward_min_device};
    const int blocks = (num_episodes + bn::kScoreThreads - 1) / bn::kScoreThreads;
    bn::episode_score_kernel<<<blocks, bn::kScoreThreads, 0, (hipStream_t)stream>>>(states_device, rewards_device, goals_device, end_step_device,
                                                                                   done_step_device, stopped_device, invalid_device, n_steps,
                                                                                   num_episodes, stuck_threshold, delta_t, o);
    BN_HIP_OR(score_fail, hipGetLastError());
    return BN_OK;
}

}  // extern "C"
