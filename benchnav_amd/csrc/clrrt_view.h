// clrrt_view.h -- what the CL-RRT plan-follow-replan loop (bn_clrrt_loop_run, clrrt_loop.hip) reads and drives of a CL-RRT handle,
// and the launch interface of its follow kernel.  Library-internal (clrrt_kernels.hip implements the view and the masked replan,
// clrrt_loop.hip the follow kernel); not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/benchnav_mppi.h"
#include "episode_rows.h"
#include "mppi_kernels.h"

struct bn_clrrt;

namespace bn {

constexpr int kClrrtFollowThreads = 256;
constexpr int kClrrtFollowLdsStates = 8192;    // planned (x, y) pairs staged in LDS: 64 KB; a longer plan is read from global memory
constexpr int kClrrtResultWords = 6;           // words of a row of BN_CLRRT_BUF_RESULTS (== clrrt_kernels.hip's kClrrtResult)

struct ClrrtView {
    bn_clrrt_config cfg;
    int device, B, iters, path_cap;
    bool have_map;
    float *starts;              // (B, 3) the states the next masked plan starts from (the follow kernel fills the rows it flags)
    float *goals;               // (B, 3) goal nodes
    float *samples;             // (B, iters, 3)
    float *path_actions;        // (B, path_cap, 2)
    float *path_states;         // (B, path_cap + 1, 3)
    const int32_t *results;     // (B, kClrrtResultWords): found, pick, length, near-goal count, error, node count
};

int clrrt_view(bn_clrrt *h, ClrrtView *v);
// A new episode: the goal nodes (B, 3) and the seeds (B) of the instances' MT19937 streams, HOST arrays consumed before the call
// returns; the streams are seeded on `s` and continue across the masked plans that follow.
int clrrt_loop_reset(bn_clrrt *h, hipStream_t s, const float *goal_nodes, const uint64_t *seeds);
// One plan on `s` for the instances whose `active` word (device, (B)) is non-zero, from the device rows of `starts`: samples from the
// streams (draw != 0) or the rows already in `samples`, then growth, pick and path.  An inactive instance keeps every byte.
int clrrt_plan_masked(bn_clrrt *h, hipStream_t s, const int32_t *active, int draw);

// the loop's per-rover words, as the device holds them
struct ClrrtRover {
    int32_t iter;        // loop iterations since the reset
    int32_t status;      // bn_clrrt_loop_status
    int32_t need;        // 0 following a plan; 1 a plan is needed (flagged, or none yet); 2 requested from the planner: the next launch takes it
    int32_t aidx;        // action_index
    int32_t length;      // L of the current plan
    int32_t plans;       // planner plans taken since the reset
    int32_t steps;       // environment steps since the reset
    int32_t done_iter;   // the iteration at which the status was set, or -1
};

struct ClrrtFollowArgs {
    ClrrtRover *rover;            // (B)
    float *state;                 // (B, 3) in/out
    float *starts;                // (B, 3) the planner's start rows
    const float *goal_nodes;      // (B, 3)
    const float *path_actions;    // (B, path_cap, 2)
    const float *path_states;     // (B, path_cap + 1, 3)
    const int32_t *results;       // (B, kClrrtResultWords)
    int32_t *active;              // (B) the replan mask
    int32_t *pending;             // rovers that asked for a plan in this launch
    float *psamples;              // (B, iters, 3) the planner's sample rows
    const float *inj;             // (P, B, iters, 3) injected sample tables, or nullptr
    int P, iters, path_cap;
    EpisodeRows log;              // rows by iteration of the call
    float *log_dev;               // (cap, B)
    int32_t *log_plan;            // (cap, B)
    int32_t *log_event;           // (cap, B)
    const float *z;               // (n, B) injected slip draws of the call's iterations, or nullptr
    int32_t iter0, n;             // the call runs the episode's iterations [iter0, iter0 + n)
    int32_t limit_steps;          // the step count at which the float64 sum of delta_t exceeds the time limit
    int32_t use_lds;              // stage the plan's positions in LDS when they fit
    double xlo, xhi, ylo, yhi;    // the planner's limits (forward's bounds test)
};

hipError_t launch_clrrt_follow(const SolveParams &p, const ClrrtFollowArgs &a, hipStream_t s);

// What a run leaves of the rovers' words for readers on the device, (B) int32 each, one column behind the other:
//   done_step  done_iter where the status is BN_CL_GOAL, else -1           (bn_episode_score's done_step)
//   stopped    the status where it is neither RUNNING, GOAL nor TIME_LIMIT, else 0      (... and its stopped)
//   status, plans  the rover's own words
struct ClrrtOutcome {
    int32_t *w;
    size_t B;
    static size_t count(size_t B) { return 4 * B; }
    __host__ __device__ int32_t *done_step() const { return w; }
    __host__ __device__ int32_t *stopped() const { return w + B; }
    __host__ __device__ int32_t *status() const { return w + 2 * B; }
    __host__ __device__ int32_t *plans() const { return w + 3 * B; }
};
hipError_t launch_clrrt_outcome(const ClrrtRover *rover, const ClrrtOutcome &out, hipStream_t s);

}  // namespace bn
