/*
 * benchnav_mppi.h -- C ABI of the MI355X-native MPPI local planner.
 *
 * This is the drop-in boundary for BenchNav's MPPI hot path.  The reference has
 * no FFI layer: its boundary is the Python class
 *     src/planners/local_planners/mppi.py:17   class MPPI(nn.Module)
 * whose methods the entry points below replace one for one (citations are
 * reference file:line).  The Python mirror of that class lives in
 * benchnav_amd/mppi.py and binds these symbols with ctypes; INTEGRATION.md shows
 * the stub a BenchNav maintainer would add.
 *
 * Conventions
 *   - plain C types only; every function returns BN_OK (0) or a negative bn_status,
 *     bn_last_error() gives the message of the calling thread's last failure;
 *   - a handle is bound to one HIP device and one HIP stream; it is not
 *     thread-safe, distinct handles are independent;
 *   - "host"/"device" in a parameter name says where the pointer must live;
 *     the library owns every device buffer it allocates, callers own theirs;
 *   - all arrays are float32, C-contiguous; shapes use the reference's names:
 *     K = num_samples, T = horizon, G = grid_size, B = num_instances;
 *   - `*_async` entry points only enqueue work on the handle's stream.
 */
#ifndef BENCHNAV_MPPI_H
#define BENCHNAV_MPPI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BN_MPPI_ABI_VERSION 7

typedef enum bn_status {
    BN_OK = 0,
    BN_ERR_INVALID = -1,      /* bad argument / unsupported configuration          */
    BN_ERR_HIP = -2,          /* a HIP runtime call failed (message has the detail) */
    BN_ERR_NO_DEVICE = -3,    /* no usable gfx950 device                            */
    BN_ERR_STATE = -4         /* call sequence error (e.g. solve before set_map)    */
} bn_status;

/* Where the per-solve standard-normal noise eps comes from (mppi.py:149-151). */
typedef enum bn_noise_kind {
    BN_NOISE_PHILOX = 0,      /* generated in the rollout kernel (Philox4x32 + Box-Muller: eight rounds for the per-rollout streams) */
    BN_NOISE_HOST_KT2 = 1,    /* host pointer, (B,K,T,2): the reference's rsample layout       */
    BN_NOISE_DEVICE_KT2 = 2,  /* device pointer, (B,K,T,2)                                      */
    BN_NOISE_DEVICE_T2K = 3   /* device pointer, (B,T,2,K): planner-native, coalesced           */
} bn_noise_kind;

typedef enum bn_mem_kind { BN_MEM_HOST = 0, BN_MEM_DEVICE = 1 } bn_mem_kind;

/* Device buffers a caller may map without a copy (bn_mppi_device_buffer). */
typedef enum bn_buffer_id {
    BN_BUF_STATES = 0,    /* (B,T+1,3,Kp) _state_seq_batch, planner-native layout: k fastest, rows pitched to
                             Kp = 64*ceil(K/64) floats (bn_mppi_row_pitch)                          */
    BN_BUF_WEIGHTS = 1,   /* (B,K)        _weights                                             */
    BN_BUF_COSTS = 2,     /* (B,K)        per-rollout total cost                               */
    BN_BUF_CONTROLS = 3,  /* (B,T,2,Kp)   _perturbed_action_seqs (only with BN_FLAG_STORE_CONTROLS) */
    BN_BUF_USTAR = 4,     /* (B,T,2)      optimal_action_seq                                   */
    BN_BUF_XSTAR = 5,     /* (B,T+1,3)    optimal_state_seq                                    */
    BN_BUF_MEAN = 6,      /* (B,T,2)      _previous_action_seq                                 */
    BN_BUF_MAP = 7,       /* (n_maps,G,G) risk map(s)                                          */
    BN_BUF_GOAL = 8,      /* (B,2)                                                             */
    BN_BUF_USTAR_XSTAR = 9, /* the (B,T,2) U* block followed by the (B,T+1,3) X* block: both outputs of forward() are one
                               contiguous allocation, so a caller that wants private copies makes ONE device copy     */
    BN_BUF_STATES_ALT = 10,   /* the second (B,T+1,3,Kp) / (B,T,2,Kp) buffers of handles that overlap launches (bn_mppi_states_buffer_index) */
    BN_BUF_CONTROLS_ALT = 11,
    BN_BUF_COUNT_ = 12
} bn_buffer_id;

enum {
    BN_FLAG_STORE_CONTROLS = 1u << 0,  /* materialise _perturbed_action_seqs in HBM          */
    BN_FLAG_SHARED_MAP = 1u << 1,      /* all B instances plan on map 0                      */
    BN_FLAG_NO_LDS_WINDOW = 1u << 2,   /* debug: gather the risk map from global memory      */
    BN_FLAG_PROFILE = 1u << 3,         /* record HIP events around each kernel (see bn_mppi_kernel_ms) */
    BN_FLAG_PRIVATE_STREAM = 1u << 4,  /* ignore `stream`: the library creates and owns a non-blocking stream */
    BN_FLAG_NO_PIPELINE = 1u << 5,     /* always two launches per solve (rollout, finish); see bn_mppi_solve_async */
    BN_FLAG_WAVE_KERNEL = 1u << 7,     /* always use the one-wave-per-64-rollouts throughput kernel (default: chosen by launch size) */
    BN_FLAG_ROLE_KERNEL = 1u << 8,     /* always use the five-wave role-split latency kernel */
    BN_FLAG_NO_OVERLAP = 1u << 11,     /* bn_mppi_solve_n_async keeps all its launches on the handle's stream (default: with the latency
                                          kernel consecutive solves alternate between two streams and overlap, see there) */
    BN_FLAG_LAT_KERNEL = 1u << 10,     /* always use the barrier-free latency variant of the role kernel when it fits (default: when the
                                          launch leaves every workgroup a CU to itself) */
    BN_FLAG_LEAN = 1u << 9,            /* lean mode: _state_seq_batch (mppi.py:119-125) is not materialised -- 70 % of a solve's
                                          HBM bytes; bn_mppi_get_states / bn_mppi_get_top_samples / bn_mppi_reroll_async
                                          regenerate the requested rows of the latest solve bit-identically on demand */
    BN_FLAG_SAMPLED_SLIP = 1u << 6,    /* BASELINE config 3: every traversability lookup of the rollouts draws
                                          slip ~ Normal(map, slip_std)[cell]; see bn_mppi_set_slip_std */
    BN_FLAG_HOST_PACED = 1u << 13,     /* opt-in for a host loop that calls bn_mppi_forward_state_async once per control step and consumes every solve's
                                          first action (test_mppi.py:174-181): the launch of the NEXT solve is enqueued one step ahead and waits on
                                          the device for the state the next call posts -- see bn_mppi_forward_state_async.  One instance, latency
                                          kernel, num_samples <= 1024, Philox noise; bn_mppi_host_paced() tells whether the handle qualifies */
    BN_FLAG_UNORDERED_OUTPUTS = 1u << 14, /* with BN_FLAG_HOST_PACED, for a loop that consumes the first action and rarely anything else: the steady-state
                                          bn_mppi_forward_state_async does NOT order the handle's stream behind the posted solve (3-5 us of host
                                          time per control step).  Every other entry point of the handle (bn_mppi_first_action and the pure queries
                                          aside) makes up for it when it is called; a caller that enqueues its OWN consumers of `out_device` or of
                                          the device buffers calls bn_mppi_order_outputs first */
    BN_FLAG_REFERENCE_ORDER = 1u << 12 /* the transit in the REFERENCE's own operation order, robot_model.py:75-95: sin / cos of every
                                          step's heading, x + ((trav v) cos) dt, theta + (trav omega) dt, the general heading wrap.
                                          The default arithmetic (heading vector carried by a rotation per step, one fused update) leaves
                                          positions 1-2 ulp from the reference's, and about one rollout in 30 000 (T = 50; one in 7 000 at
                                          T = 100) then lands in a neighbouring cell and leaves the 1e-4 trajectory tolerance from there on
                                          (tests/golden/census_*.npz); with this flag none did in 0.7 M rollouts at T = 50 and
                                          one in 0.7 M at T = 100 -- the level of libm against the reference's own SLEEF.  Every kernel has
                                          an instantiation in this arithmetic; the price is the chain's extra instructions: 10.8 instead of
                                          8.0 us per dependent single-instance solve, 1-8 % for batched launches and K > 4096 (DESIGN.md
                                          4.15).  dt * max|omega| > 0.5 selects this arithmetic
                                          by itself).  bn_mppi_arithmetic() tells which arithmetic a handle runs. */
};

/*
 * Everything MPPI.__init__ (mppi.py:23-128) receives or reads from its
 * `dynamics` / `objectives` arguments, flattened to plain data:
 *   horizon, num_samples              mppi.py:25-26
 *   sigma                             mppi.py:31,89
 *   inv_var = diag(inverse(diag(sigma^2)))   mppi.py:94-97 (host computes it the reference's way)
 *   lambda_                           mppi.py:32,90
 *   u_min, u_max                      robot_model.py:54-57 via mppi.py:83-88
 *   dt                                robot_model.py:60 (transit's default delta_t = 0.1)
 *   stuck_threshold                   objectives.py:27
 *   grid_size, resolution, x/y_limits grid_map.py:40-50  (limits[0] is also the index origin, grid_map.py:199-201)
 */
typedef struct bn_mppi_config {
    uint32_t struct_size;     /* = sizeof(bn_mppi_config) */
    int32_t device_id;        /* HIP device ordinal */
    int32_t horizon;          /* T >= 1 */
    int32_t num_samples;      /* K >= 1 */
    int32_t num_instances;    /* B >= 1 independent planning instances solved per call */
    int32_t grid_size;        /* G >= 1 */
    float resolution;
    float x_limits[2];
    float y_limits[2];
    float sigma[2];
    float inv_var[2];
    float lambda_;
    float u_min[2];
    float u_max[2];
    float dt;
    float stuck_threshold;
    uint64_t seed;            /* Philox key for BN_NOISE_PHILOX */
    uint32_t flags;           /* BN_FLAG_* */
    void *stream;             /* hipStream_t to enqueue on; NULL is HIP's default (null) stream, which is
                                 also torch's default stream.  See BN_FLAG_PRIVATE_STREAM. */
} bn_mppi_config;

typedef struct bn_mppi bn_mppi_t;

/* Fills *cfg with the reference's defaults (robot_model.py:54-60, test_mppi.py:160-169). */
void bn_mppi_config_init(bn_mppi_config *cfg);

/* MPPI.__init__, mppi.py:23-128: allocates the device buffers (_state_seq_batch,
 * _weights, _previous_action_seq = 0, ...).  Fails with BN_ERR_NO_DEVICE when no
 * gfx950 device is present: there is no CPU fallback. */
int bn_mppi_create(const bn_mppi_config *cfg, bn_mppi_t **out);
void bn_mppi_destroy(bn_mppi_t *h);

/* dynamics._traversability_model._risks (traversability_model.py:24-26), (G,G)
 * row-major [iy][ix] (grid_map.py:167).  instance = -1 sets every map. */
int bn_mppi_set_map(bn_mppi_t *h, int32_t instance, const float *risk, bn_mem_kind where);
/* Sampled-slip mode (BN_FLAG_SAMPLED_SLIP): the map set with bn_mppi_set_map is the slip MEAN and this the slip
 * STD per cell, (G,G); every get_traversability of the rollouts then evaluates 1 - clamp(z*std + mean, 0, 1) with
 * a fresh standard normal z (the observation-mode branch, traversability_model.py:65-69): T draws in transit,
 * T+1 in the stage/terminal costs per rollout, T in the optimal rollout.  The reference's own MPPI cannot run in
 * this mode; the semantics are those of its components. */
int bn_mppi_set_slip_std(bn_mppi_t *h, int32_t instance, const float *std, bn_mem_kind where);
/* Optional injected draws for the next solves (device pointers, k fastest): transit (B,T,K), cost (B,T+1,K),
 * optimal rollout (B,T).  NULL (default) = the library's Philox stream. */
int bn_mppi_set_slip_noise(bn_mppi_t *h, const float *zt_device, const float *zc_device, const float *zo_device);
/* objectives._goal_pos (objectives.py:26).  instance = -1 sets every instance. */
int bn_mppi_set_goal(bn_mppi_t *h, int32_t instance, const float goal_host[2]);
/* _previous_action_seq (mppi.py:116,217): (T,2) host array; NULL resets it to zero. */
int bn_mppi_set_mean(bn_mppi_t *h, int32_t instance, const float *mean_host);
int bn_mppi_get_mean(bn_mppi_t *h, int32_t instance, float *mean_host);

/*
 * MPPI.forward(state), mppi.py:130-219, for all B instances.
 *   states   (B,3) current states, host or device per `states_where`
 *   eps      noise per `noise` (NULL for BN_NOISE_PHILOX)
 *   ustar_host  (B,T,2)    optimal_action_seq, may be NULL
 *   xstar_host  (B,T+1,3)  optimal_state_seq,  may be NULL
 * Synchronous like the reference: returns after the stream has drained and the
 * outputs are in the host arrays.  Updates _previous_action_seq (no shift, mppi.py:217).
 */
int bn_mppi_solve(bn_mppi_t *h, const float *states, bn_mem_kind states_where, const float *eps,
                  bn_noise_kind noise, float *ustar_host, float *xstar_host);
/* Same, enqueue only: results stay in the device buffers (bn_mppi_device_buffer).
 * For K <= 2048 consecutive async solves are software-pipelined: the launch of solve i also merges
 * solve i-1's softmin statistics (its warm start) and writes solve i-1's U*, X* and weights, so a
 * dependent chain of solves costs one launch each.  bn_mppi_sync, bn_mppi_solve and every getter
 * first write the pending tail of the latest solve; device buffers obtained with
 * bn_mppi_device_buffer are up to date after bn_mppi_sync (or bn_mppi_flush + stream order). */
int bn_mppi_solve_async(bn_mppi_t *h, const float *states, bn_mem_kind states_where,
                        const float *eps, bn_noise_kind noise);
/* MPPI.forward (mppi.py:130-219) for a host loop that consumes every solve (test_mppi.py:174-183): bn_mppi_solve_async +
 * bn_mppi_flush in one call.  states_device (B,3) and eps_device are device pointers; nothing waits.  out_device (may be
 * NULL): a caller-owned device block laid out like BN_BUF_USTAR_XSTAR that the tail fills as well -- the fresh
 * (optimal_action_seq, optimal_state_seq) tensors the reference returns, without another launch. */
int bn_mppi_forward_async(bn_mppi_t *h, const float *states_device, const float *eps_device, bn_noise_kind noise,
                          float *out_device);
/* The same with the states taken from HOST memory, by value, at the call (ABI 4): the loop of test_mppi.py:174-181 whose environment
 * lives on the host has a fresh state every control step, and `state.to(device)` in front of forward() (mppi.py:140-144) is an
 * upload the solve then waits for.  states_host (B,3) may be reused as soon as the call returns.  One instance on the latency
 * kernel: the state travels in the kernel arguments -- no copy is enqueued, and the kernel's prologue has no fetch in front of its
 * window; other configurations stage and upload it (as bn_mppi_solve_async does for BN_MEM_HOST).
 * ONE LAUNCH per call (both entry points, and bn_mppi_solve) where the latency kernel serves the handle (bn_mppi_launches_per_forward):
 * the tail of the solve -- softmin merge, U*, the first-action mailbox (bn_mppi_first_action), X*, the weights -- is a workgroup of
 * the rollout launch itself that waits on the device for the rollout workgroups dispatched in front of it; results are bit-identical
 * to the two-launch path's.  That wait is bounded like every device-side wait of the library and cannot expire short of a stalled
 * GPU; if it does, the next call that concerns results returns BN_ERR_HIP (the latest solve's outputs are invalid) and the handle
 * keeps to two launches from then on. */
int bn_mppi_forward_state_async(bn_mppi_t *h, const float *states_host, const float *eps_device, bn_noise_kind noise,
                                float *out_device);
/* With BN_FLAG_HOST_PACED (and BN_NOISE_PHILOX) the call also enqueues the launch of the NEXT solve -- on a stream of the library's
 * own -- before it returns: while the host waits for this solve's first action, takes its environment step and comes back, that
 * launch gets its latency, its instruction fetch, the horizon's noise, its mean (the merge of this solve's partial rows), the whole
 * control tile and a window around THIS state (two cells wider each side) behind it and then waits, on the device, for the state the
 * next call posts to pinned host memory.  Between the host's store and the first action's way back only the rollouts' 50-step chain,
 * the cost epilogue and the merge are left: 25 -> ~14 us per control step at K = 1024, T = 50.  Results are bit-identical to the
 * one-launch path's (same noise stream positions, same merges).
 *   - outputs stay stream-ordered for what comes AFTER: every posted solve's launch is followed by an event the handle's stream waits
 *     for (BN_FLAG_UNORDERED_OUTPUTS: not before the next call that needs it, see bn_mppi_order_outputs).  What was enqueued on the handle's stream BEFORE the call is not waited for (the launch is paced by the host's store, not by
 *     the queue): work left there that still reads the planner's own buffers (BN_BUF_WEIGHTS, BN_BUF_STATES, BN_BUF_USTAR_XSTAR ...),
 *     or that still uses the memory `out_device` was carved from, must have completed -- fresh output blocks per call need nothing;
 *   - a launch that waits for a state holds 17 CUs and is cancelled -- a word in pinned memory, no synchronisation -- by every other
 *     entry point of the handle except bn_mppi_first_action and the pure queries (the next bn_mppi_forward_state_async then pays one
 *     ordinary launch); left alone it gives up after ~50 ms and the next call starts over the same way;
 *   - a DEVICE-WIDE synchronisation (hipDeviceSynchronize, torch.cuda.synchronize) issued while a launch waits blocks for up to
 *     those 50 ms: end the loop with any other call of the handle (bn_mppi_flush is the cheapest) first.  This is why the mode is
 *     opt-in;
 *   - a state more than two cells from the previous one (a reset) is handled inside the waiting launch (it stages its window again). */
/* BN_FLAG_UNORDERED_OUTPUTS: order the handle's stream behind the latest posted solve (one stream-wait; a no-op when that has been done
 * or the flag is not set).  Does not cancel the launch that waits for the next state: the loop keeps its pace. */
int bn_mppi_order_outputs(bn_mppi_t *h);
int32_t bn_mppi_host_paced(const bn_mppi_t *h);      /* 0: no; 1: BN_FLAG_HOST_PACED was given and the handle qualifies; 2: ... and the request words live in
                                                         device memory the host writes through the PCIe BAR (no PCIe read on the launch's side) */
/* Which of the two trajectory / control buffers holds the LATEST solve (0: BN_BUF_STATES / BN_BUF_CONTROLS, 1: the *_ALT ones): host-paced
 * solves alternate between them (two launches are in flight and must not write the same addresses); every other path writes buffer 0. */
int32_t bn_mppi_states_buffer_index(const bn_mppi_t *h);
/* n dependent solves enqueued from one call (the warm start chains them on the device; the state is
 * re-read from `states` by every solve).  Noise block i is eps + (i % eps_ring) * eps_stride floats.
 * With n >= 3 (and device-resident inputs) the solves of one call alternate between the handle's stream and an internal one and
 * OVERLAP: solve i+1 is dispatched while solve i runs and waits on the device for its predecessor's softmin partials instead of
 * for its kernel's end; results are bit-identical to the one-stream chain (BN_FLAG_NO_OVERLAP turns it off: the switch for a GPU
 * shared with other work).  Several handles in one process: a batch overlaps only while every other handle on the device is idle,
 * and a launch of another handle that arrives while an overlapped batch is in flight runs behind that batch's end (events on the
 * device, no host blocking) -- waiting workgroups hold their slots and must not share the device with anybody's launches.
 * What is ordered for the caller:
 *   - the LAST solve of the call and the tail behind it run on the handle's stream, so work enqueued there afterwards is ordered
 *     behind the batch's final results by the queue itself; the internal stream is not joined back -- its kernels have handed
 *     everything over through device counters by then and end within microseconds (bn_mppi_sync waits for both);
 *   - `states` is read by every solve of the call, `eps` block i by solve i: they must stay valid and unchanged until the batch has
 *     run -- work enqueued on the handle's stream behind the call may overwrite `states` (a host-driven closed loop that keeps
 *     ONE state buffer: batch, write the next state in stream order, batch);
 *   - `eps` (caller-provided noise) must stay valid AND UNCHANGED until the synchronisation point that follows the batch
 *     (bn_mppi_sync, a getter, or the caller's own stream synchronisation): a re-run, see below, reads it again.
 * Device-side waits are bounded (~2 s: another user of the GPU kept a predecessor from becoming resident).  If one expires the
 * launch computes on incomplete partials; the error word it sets lives in pinned host memory and is looked at by EVERY entry
 * point that synchronises (bn_mppi_sync, the getters, the setters, bn_mppi_episode_log ...) and by bn_mppi_flush: the batches
 * enqueued since the last clean synchronisation point are then RE-RUN on one stream from the mean the first of them started
 * from (kept on the device), with the same Philox positions, the callers' noise buffers, and the states each batch was GIVEN: the
 * first launch of every journalled batch keeps them in memory the handle owns (ABI 3, round 4; before that a caller that rewrote
 * its state tensor in place between batches got the re-run on the new contents).
 * The call returns BN_OK with a warning in bn_last_error(), bn_mppi_recovery_count() counts these events (consumers enqueued in
 * stream order BEFORE the synchronisation point have read invalid buffers), and the handle keeps to one stream from then on.
 * BN_ERR_HIP only when the batches cannot be re-run (host-resident inputs; more than min(4096, 16 MB / (12 B x num_instances), at least 64) batches without a synchronising call).
 * Host side of the call.  "async" means the call does not wait for the solves -- but it is not free of host waits: a batch whose
 * launches exceed one residency round each (64+ instances of K = 1024 on the role kernel) hands its first three launches over one
 * by one -- the host spins on a pinned word (a few microseconds; at most 2 ms per hand-over, then it falls back to
 * hipStreamSynchronize on that launch's stream, which also waits for whatever the caller queued there before) --, and a batch of
 * such launches that finds the handle's stream busy synchronises it first.  Small launches (the single-instance path) never block.
 * Threads.  A handle is not thread-safe, and the handles of ONE device are not independent of each other while overlapped batches
 * are in use: the library orders every launch of a handle behind another handle's overlapped batch that may still be in flight
 * (solves, stand-alone tails, re-rolls, environment steps), and it decides that from host-side state it reads at the call.  Calls
 * that concern one device must therefore come from one thread at a time (the caller's lock, or one thread per device); handles on
 * different devices are independent.  BN_FLAG_NO_OVERLAP on every handle of a device lifts the restriction for those handles. */
int bn_mppi_solve_n_async(bn_mppi_t *h, int32_t n, const float *states, bn_mem_kind states_where,
                          const float *eps, bn_noise_kind noise, int32_t eps_ring, int64_t eps_stride);

/* ---- K-sharded solve (optional row): ONE solve whose K_total rollouts are split over ranks ----------
 * Every rank owns a handle with num_samples = its shard and rollouts [first_rollout, first_rollout + num_samples) of
 * the global solve (the offset keys the Philox stream, so the union of the shards draws exactly the noise of the
 * unsharded solve).  Per solve:
 *   1. bn_mppi_shard_rollout_async            rollouts + costs of the shard, per-workgroup softmin partials
 *   2. exchange                               all-gather bn_mppi_shard_partials over the ranks, rank order (RCCL)
 *   3. bn_mppi_shard_finish_async             merge ALL partials in that order (bit-identical U* on every rank and equal
 *                                             to the unsharded solve's), next mean, X*, and the shard's weights
 * The reference has no multi-GPU path; the exchange is the log-sum-exp merge of mppi.py:193-199. */
int bn_mppi_set_rollout_offset(bn_mppi_t *h, int64_t first_rollout);
int bn_mppi_shard_rollout_async(bn_mppi_t *h, const float *states, bn_mem_kind states_where, const float *eps, bn_noise_kind noise);
int bn_mppi_shard_partials(bn_mppi_t *h, const float **partials_device, int32_t *workgroups, int32_t *floats_per_workgroup);
int bn_mppi_shard_finish_async(bn_mppi_t *h, const float *all_partials_device, int32_t total_workgroups);
/* The same three steps as ONE call with the exchange enqueued by the library: RCCL's ncclAllGather on the handle's own stream
 * between the two kernels -- no host wait, no event, no second stream (what a caller driving steps 1-3 through
 * torch.distributed pays per solve).  Equal shards only (num_samples the same on every rank).  RCCL is opened with dlopen
 * on first use; nothing else in the library depends on it.
 *   bn_dist_unique_id          rank 0 draws the id (ncclGetUniqueId) and hands the 128 bytes to the other ranks by any means
 *                              (benchnav_amd.sharding broadcasts them over the torch.distributed group the job has anyway)
 *   bn_mppi_shard_comm_init    collective over the ranks of the solve (ncclCommInitRank on the handle's device); the communicator
 *                              and the buffer of gathered partial rows belong to the handle and go with bn_mppi_destroy
 *   bn_mppi_shard_solve_async  rollouts of the shard, all-gather of the partial rows (rank order), merge + tail
 * Results are those of steps 1-3 above: bit-identical on every rank and to the unsharded solve.  Ordering: U* and the next mean are
 * written on the handle's stream by the merge; X*, the shard's weights and the cost copy by a tail the library runs on a second
 * stream beside the NEXT solve's rollouts -- they are ordered on the handle's stream by the next call that concerns results
 * (bn_mppi_flush, bn_mppi_sync, any getter, bn_mppi_device_buffer), which enqueues the join without blocking the host. */
#define BN_DIST_UNIQUE_ID_BYTES 128
int bn_dist_unique_id(uint8_t out[BN_DIST_UNIQUE_ID_BYTES]);
/* Everything bn_mppi_shard_comm_init can fail on short of the collective itself, done locally (ABI 4): RCCL opened, the handle's state
 * checked, the gathered-rows buffer, the events and the side stream created.  A job calls it on every rank, agrees on the outcome
 * (one all-reduce over the process group it has anyway) and enters bn_mppi_shard_comm_init -- ncclCommInitRank, which blocks until
 * EVERY rank has entered -- only if all of them are ready.  bn_mppi_shard_comm_init calls it itself when the caller has not. */
int bn_mppi_shard_comm_prepare(bn_mppi_t *h, int32_t world_size, int32_t rank);
int bn_mppi_shard_comm_init(bn_mppi_t *h, const uint8_t unique_id[BN_DIST_UNIQUE_ID_BYTES], int32_t world_size, int32_t rank);
int bn_mppi_shard_solve_async(bn_mppi_t *h, const float *states, bn_mem_kind states_where, const float *eps, bn_noise_kind noise);
/*
 * Device-side closed loop: PlanetaryEnv.step (planetary_env.py:189-219) between consecutive solves, for
 * all B instances, without a host round trip per control step (the reference loop: test_mppi.py:171-198).
 *   env_attach   latent slip model Normal(mean, std) per cell, (n_maps,G,G) each (grid_map.distributions
 *                ["latent_models"], sampled in observation mode: traversability_model.py:65-69),
 *                goal_threshold (planetary_env.py:215-217), the environment's delta_t, Philox key.
 *   episode      n_steps control steps: solve at the current state, apply U*[0] through the observation-mode
 *                transit with a freshly sampled slip, test the goal.  Like PlanetaryEnv.step, a terminated
 *                environment keeps moving when stepped (the reference's driver loop stops instead,
 *                test_mppi.py:192-194); bn_mppi_env_set_freeze(h, 1) opts into freezing an instance once it is
 *                within goal_threshold, for fixed-length batched episodes.  z_device: optional (n_steps, B) standard normals for the slip draws (parity
 *                tests), NULL = in-kernel Philox.  One launch per control step (K <= 2048 only).
 *   episode_log  states (n_steps+1, B, 3) incl. the initial one, rewards (n_steps, B) = traversability
 *                observed by each step (planetary_env.py:209), actions (n_steps, B, 2) = the control each step
 *                applied (action_seq[0] of test_mppi.py:181), done_step (B) = first step whose resulting
 *                state lies within goal_threshold, or -1.  Any pointer may be NULL.  Synchronises.
 */
int bn_mppi_env_attach(bn_mppi_t *h, const float *latent_mean, const float *latent_std, bn_mem_kind where,
                       float goal_threshold, float delta_t, uint64_t seed);
/* The two PlanetaryEnv calls on their own, for callers that drive the loop themselves (all pointers device memory, stream-ordered):
 *   env_step             planetary_env.py:189-219 for the B environments: states (B,3) advance in place through the
 *                        observation-mode transit with actions (B,2); rewards (B,) = the sampled traversability;
 *                        terminated (B,) = within goal_threshold of the goal (a terminated environment moves on when
 *                        stepped again, as the reference's does, unless bn_mppi_env_set_freeze).  z (B,) injects the slip draws, NULL = Philox keyed by
 *                        (env seed, step_index).
 *   env_collision_check  planetary_env.py:221-232: out (B,N) = sampled traversability at states (B,N,3) <= stuck_threshold,
 *                        one fresh draw per position (z (B,N) injects them; NULL = Philox keyed by (env seed, draw_index)). */
int bn_mppi_env_set_freeze(bn_mppi_t *h, int32_t freeze_on_goal);      /* default 0 = the reference's behaviour */
int bn_mppi_env_step(bn_mppi_t *h, const float *actions_device, float *states_device, float *rewards_device,
                     int32_t *terminated_device, const float *z_device, uint64_t step_index);
int bn_mppi_env_collision_check(bn_mppi_t *h, const float *states_device, int32_t n_positions, float stuck_threshold,
                                const float *z_device, uint64_t draw_index, uint8_t *out_device);
int bn_mppi_episode_async(bn_mppi_t *h, int32_t n_steps, const float *states0, bn_mem_kind states_where,
                          const float *eps, bn_noise_kind noise, int32_t eps_ring, int64_t eps_stride,
                          const float *z_device);
int bn_mppi_episode_log(bn_mppi_t *h, float *states_host, float *rewards_host, float *actions_host,
                        int32_t *done_step_host);
/* Device views of the latest episode's log, for a consumer on the handle's stream (bn_episode_score): states (n_steps + 1, B, 3),
 * rewards (n_steps, B), done_step (B), valid until the next episode; row_capacity is the rows the buffers were allocated for.
 * Any pointer may be NULL.  Nothing is copied. */
int bn_mppi_episode_buffers(bn_mppi_t *h, const float **states_device, const float **rewards_device, const int32_t **done_step_device,
                            int32_t *n_steps, int32_t *row_capacity);
/*
 * DWA.forward(state), reference src/planners/local_planners/dwa.py:116-153, on the planner handle's map, goal and
 * geometry.  The caller supplies the dynamic-window candidates (dwa.py:168-199: cartesian_prod of two linspaces),
 * (B, num_actions, 2) constant (v, omega) pairs; each is rolled out `horizon` steps with the MPPI transit/aliasing
 * (dwa.py:224-227), costed against `stage_goal` (the sub-goal of dwa.py:260-285, NULL = the goal) per stage and
 * against the goal at the end, summed in fp32 in step order (dwa.py:251-256).
 *   best_action (B,2), best_states (B,T+1,3): the argmin candidate (first minimum)        dwa.py:139-143
 *   costs, weights (B,num_actions): cost_batch and softmax(-cost_batch)                    dwa.py:151
 *   states_all (B,num_actions,T+1,3): _state_seq_batch; best_index (B).  Any output may be NULL.  Synchronous.
 */
int bn_mppi_dwa_solve(bn_mppi_t *h, const float *states_host, const float *actions_host, int32_t num_actions,
                      const float *stage_goal_host, float *best_action_host, float *best_states_host,
                      float *costs_host, float *weights_host, float *states_all_host, int32_t *best_index_host);
/* Device-resident outputs of the latest bn_mppi_dwa_solve with this num_actions (valid until the next call that uses the
 * handle's scratch memory): states_all (B,num_actions,T+1,3), costs and weights (B,num_actions). */
int bn_mppi_dwa_buffers(bn_mppi_t *h, int32_t num_actions, const float **states_all_device, const float **costs_device,
                        const float **weights_device);
/* DWA.forward with nothing on the host (dwa.py:116-153 incl. _generate_actions :168-199 and the sub-goal of :240-244,
 * 260-285): the window grid around prev_action_device (B,2) -- linspace x linspace, v major -- and the sub-goal on
 * path_device (num_path,2; NULL: the goal) are computed on the device, the sub-goal like the reference from candidate 0's
 * aliased slot-0 state; then the candidates are rolled out and costed as in bn_mppi_dwa_solve.  Only enqueues.
 * prev_action_device is updated in place with the argmin action (dwa.py:147: the next window's centre) -- it IS
 * optimal_action_seq; best_states_device (B,T+1,3) may be NULL.  The candidate batch stays in the handle's scratch:
 * bn_mppi_dwa_buffers (states, costs, weights) and bn_mppi_dwa_candidates (the window grid and the sub-goal used). */
int bn_mppi_dwa_forward_async(bn_mppi_t *h, const float *states_device, float *prev_action_device, const float a_lim_host[2],
                              float dwa_delta_t, int32_t num_lin_vel, int32_t num_ang_vel, const float *path_device, int32_t num_path,
                              float lookahead, float *best_states_device);
int bn_mppi_dwa_candidates(bn_mppi_t *h, int32_t num_actions, const float **actions_device, const float **stage_goal_device);
/* Write the pending tail, wait for the handle's stream, check the overlapped launches' error word (see bn_mppi_solve_n_async). */
int bn_mppi_sync(bn_mppi_t *h);
/* optimal_action_seq[0] (mppi.py:219 -> test_mppi.py:181: what env.step consumes) of the latest solve, on the host, as early as it
 * exists: the tail of a solve posts U*[0] to pinned host memory right after the softmin merge -- before it rolls out X* and
 * normalises the weights -- and this call polls for it.  No stream synchronisation, no device-to-host copy; the other outputs are
 * complete in stream order as always.  Enqueues the pending tail first (like every getter). */
int bn_mppi_first_action(bn_mppi_t *h, int32_t instance, float action_host[2]);
/* How many times this handle re-ran batches after an expired device-side wait (0 in normal operation). */
uint64_t bn_mppi_recovery_count(const bn_mppi_t *h);
/* Which way bn_mppi_solve_n_async runs its batches (ABI 4).  Overlapped launches assume the DEVICE TO THEMSELVES: the workgroups of
 * launch i+1 wait, resident, for launch i's partials, and with another process's kernels on the GPU those waiting workgroups hold the
 * slots launch i's stragglers need -- the chain then runs at half the one-stream rate (and, in the extreme, a bounded wait expires:
 * see above).  The handle protects itself: it measures its own cadence over windows of 64 launches (the first-action mailbox counts
 * finished solves; no event, no kernel change), looks at the other mode once, keeps the faster one, looks again when its cadence
 * degrades by half and -- while on one stream -- every 256 windows.
 *   0  overlapped (two streams)      1  one stream, by the handle's own choice (somebody else is on the device)
 *   2  one stream for good: a device-side wait expired once (bn_mppi_recovery_count)      3  the handle never overlaps (flags, kernel family) */
int32_t bn_mppi_overlap_mode(const bn_mppi_t *h);
/* Test hook: feed the tuner a cadence (microseconds per launch) measured in `mode` (0 overlapped, 1 one stream); returns 1 when the
 * next long batch will look at the other mode. */
int bn_mppi_debug_cadence(bn_mppi_t *h, int32_t mode, double us_per_launch);
/* Test hook: behave as if a bounded device-side wait had expired in the batches enqueued since the last synchronisation point
 * (what happens when another process keeps a launch's predecessor from becoming resident for ~2 s): sets the error word and
 * overwrites what those batches wrote (mean, U* | X*, weights, costs, trajectories) with NaN patterns.  The next synchronising
 * call re-runs them on one stream. */
int bn_mppi_debug_expire_wait(bn_mppi_t *h);
/* Test hook (BN_FLAG_HOST_PACED): how many looks of ~2 us a prelaunched solve waits for its state before it gives up (default 25000), and
 * whether bn_mppi_forward_state_async posts the state without checking that the launch is still waiting. */
int bn_mppi_debug_host_paced(bn_mppi_t *h, int32_t polls, int32_t post_unchecked);
/* Test hook: what bn_mppi_create would decide for `cfg` on a device of `n_cus` compute units -- the derived kernel parameters, the
 * launch policy, which conditional buffer groups exist, and what bn_mppi_device_buffer would report per bn_buffer_id -- without
 * touching a device.  Set out->struct_size first.  Returns what bn_mppi_create returns for a configuration it refuses. */
typedef struct bn_mppi_plan_info {
    uint32_t struct_size;
    int32_t n_cus;
    int32_t nblk, Kp, pow2, reach, WN, lds_park, ref_order, wrap_near, regen_steps, park_steps, xs, map_stride, slip_on;
    float inv_lambda;
    int32_t n_maps, slow_path, want_wave, pipelined, wave_kernel, lat_kernel, role_overlap, ticket_det, ticket_overlap, ticket_mode,
        may_overlap, n_streams;
    /* the conditional buffer groups: the trajectory batch (not in lean mode) | the control batch (requested, or where the one-wave
     * kernel keeps its controls) | granule copies of the partial rows (latency kernel, K <= 1024) | second trajectory / control
     * buffers, the journal's snapshots and the events of handles that may overlap | ticket-merge outputs, counters, group rows */
    int32_t has_X, has_U, has_granules, has_alt, has_ticket_buffers, has_slip_std;
    uint64_t snap_cap, resident_wgs;
    uint64_t buffer_bytes[12];   /* by bn_buffer_id; 0: CONTROLS and the *_ALT buffers where this configuration has none (STATES keeps
                                    its size in lean mode: what the batch would take) */
} bn_mppi_plan_info;
int bn_mppi_debug_plan(const bn_mppi_config *cfg, int32_t n_cus, bn_mppi_plan_info *out);
/* Test hook: what the solve path decided for every kernel launch it made -- the launch decision of csrc/mppi_launch.h as plain
 * numbers, buffers by identity, never an address and nothing that is the machine's answer and not the policy's.  A call with
 * out == NULL turns recording on and clears the log; every later call copies out, oldest first, the records made since the previous
 * call (at most `cap`) and returns how many.  The log is a ring of 256 records: the oldest are overwritten.  While recording is off
 * (every handle starts that way) a launch pays one predictable branch. */
typedef struct bn_mppi_launch_record {
    int32_t call;        /* who launched: 0 a solve (bn_mppi_solve*, forward), 1 a member of an overlapped batch, 2 a stand-alone tail
                            (flush), 3 a host-paced prelaunch, 4 the rollouts of a K-sharded solve */
    int32_t entry;       /* 0 launch_rollout  1 launch_rollout_lat_self  2 launch_rollout_lat_host  3 launch_rollout_lat_host_ref
                            4 launch_rollout_sampled  5 launch_finish */
    int32_t family;      /* entry 0: 0 role kernel, 1 one-wave kernel, 2 latency kernel; else 0 */
    int32_t eps_mode;    /* 0 Philox, 1 (K,T,2), 2 (T,2,K) */
    int32_t stream;      /* 0 the handle's stream, 1 / 2 its extra (host-paced: private) streams */
    int32_t have_prev, mean_from_part, self_tail, overlap, cur_slot, prev_slot;
    int32_t wave_kernel, lat_kernel, aux_prio, tail_merged, closed_loop, env_on, ep_index, state_inline, host_paced;
    int32_t x_buf;       /* trajectories: 0 the exposed buffer (or none: lean mode), 1 / 2 the alternates */
    int32_t u_buf;       /* controls: -1 none, 0 the exposed buffer, 1 / 2 the alternates */
    int32_t flag_part, flag_tail, gran, gran_prev, mean_snap, state_snap, err, err_dev, out_copy_self, env_z;   /* the pointer is set */
    int32_t part_gathered;   /* the partial rows go straight into the gathered rows of a K-sharded solve */
    uint64_t solve, tail_solve, wait_part, wait_tail, wait_part_self, wait_tail_self;   /* as in the kernel arguments; solve is 0 in the
                                                                                           record of a stand-alone tail */
} bn_mppi_launch_record;
int bn_mppi_debug_launch_log(bn_mppi_t *h, bn_mppi_launch_record *out, int32_t cap);
/* Enqueue the pending tail (if any) without waiting.  An expiry that has already been flagged is repaired here (that does wait). */
int bn_mppi_flush(bn_mppi_t *h);

/* Copies of the planner state in the REFERENCE's layouts (host arrays).  All
 * synchronise the stream first.
 *   weights  (K,)        _weights                 mppi.py:193
 *   costs    (K,)        `costs` local            mppi.py:186-190
 *   states   (K,T+1,3)   _state_seq_batch         mppi.py:119-125 (aliased slots)
 *   controls (K,T,2)     _perturbed_action_seqs   mppi.py:155-157 (needs BN_FLAG_STORE_CONTROLS)
 *   noise    (K,T,2)     eps of solve number `solve_index` regenerated from the Philox stream */
int bn_mppi_get_weights(bn_mppi_t *h, int32_t instance, float *out_host);
int bn_mppi_get_costs(bn_mppi_t *h, int32_t instance, float *out_host);
int bn_mppi_get_states(bn_mppi_t *h, int32_t instance, float *out_host);
int bn_mppi_get_controls(bn_mppi_t *h, int32_t instance, float *out_host);
/* The library's noise streams (BN_NOISE_PHILOX).  Each 128-bit block is Philox4x32-R (Random123 constants) of a counter
 * {c0, c1, c2, c3} under a key {k0, k1}; its words (x, y) and (z, w) become two normals each by Box-Muller:
 * u1 = fl(a) 2^-32 + 2^-33 in (0, 1], u2 = fl(b) 2^-32 revolutions, (z0, z1) = sqrt(-2 ln u1) (cos, sin)(2 pi u2) (a >= 0xffffff80
 * gives u1 = 1, so z = 0; a = 0 gives the largest radius, sqrt(66 ln 2) = 6.7637).  k is the global rollout index (k + the
 * rollout offset of bn_mppi_set_rollout_offset), b the instance, s the solve index, seed the config's seed:
 *   control noise  R = 8   {k, t/2, lo(s) ^ (b << 20), hi(s) ^ (b >> 12)}   key (lo(seed), hi(seed))
 *                  block (k, p) holds the (v, omega) noise of steps 2p and 2p + 1; the second half is dropped for odd T
 *   slip draws     R = 8   the same counter with t/2 -> j                     key (lo(seed) ^ 0x534c4950, hi(seed))
 *                  block (k, j): transit draws of steps 2j, 2j + 1 (x, y), cost draws of slots 2j, 2j + 1 (z, w); the optimal
 *                  rollout uses k = 0xffffffff (no offset), its block j holds the transit draws of steps 4j .. 4j + 3
 *   risk map       R = 10  {cell, i4, 0x5249534b, 0}                         key (lo(seed), hi(seed)): sample 4 i4 + s of cell
 *   env step       R = 10  {b, lo(step), hi(step), 0x454e5631}               key env seed: z = the cosine of words (x, y)
 *   collision      R = 10  {lo(i), hi(i), lo(draw), 0x434f4c4c ^ hi(draw)}   key env seed: i = b N + n, z = the cosine of (x, y)
 * The instance enters the counter by xor: instance b at solve s draws exactly what instance b' draws at solve s ^ ((b ^ b') << 20).
 * Within 2^20 consecutive solves of one handle no two instances share a block; an instance never repeats one.
 * bn_mppi_get_philox_noise regenerates the control noise of solve `solve_index` (K,T,2) with the kernels' own functions. */
int bn_mppi_get_philox_noise(bn_mppi_t *h, int32_t instance, uint64_t solve_index, float *out_host);
/* Sampled-slip mode: regenerate the library's slip draws of solve `solve_index` in the oracle's layout:
 * transit (K,T), cost (K,T+1), optimal rollout (T); rows keyed by rollout k + the rollout offset, as the solve drew them. */
int bn_mppi_get_slip_noise(bn_mppi_t *h, int32_t instance, uint64_t solve_index, float *zt_host, float *zc_host, float *zo_host);

/* MPPI.get_top_samples(n), mppi.py:221-240: the n highest-weight rollouts, sorted
 * by weight descending.  states_host (n,T+1,3), weights_host (n,).  n <= K. */
int bn_mppi_get_top_samples(bn_mppi_t *h, int32_t instance, int32_t n, float *states_host,
                            float *weights_host);

/* Rows of the LATEST solve's _state_seq_batch regenerated on the device (works in every mode but sampled-slip; it is how
 * lean mode serves get_top_samples, mppi.py:232-238): rollouts idx_device[0..n) (NULL: rollouts 0..n-1) -> out_device
 * (n,T+1,3), bit-identical to the rows a full-API solve stores (same noise, mean, start state, device functions).
 * Writes the pending tail first; with injected noise the caller's eps block of that solve must still be alive.
 * BN_ERR_STATE after a bn_mppi_set_map that followed the latest solve: the rows would be rolled out on the NEW map, not be that
 * solve's rollouts (in lean mode this also applies to bn_mppi_get_states / bn_mppi_get_top_samples). */
int bn_mppi_reroll_async(bn_mppi_t *h, int32_t instance, const int32_t *idx_device, int32_t n, float *out_device);

/* Zero-copy access to a library-owned device buffer (layouts in bn_buffer_id). */
int bn_mppi_device_buffer(bn_mppi_t *h, bn_buffer_id id, void **device_ptr, size_t *bytes);

/* Row pitch Kp (in floats) of BN_BUF_STATES / BN_BUF_CONTROLS. */
int32_t bn_mppi_row_pitch(const bn_mppi_t *h);

/* Number of solves enqueued so far (the Philox stream position). */
uint64_t bn_mppi_solve_count(const bn_mppi_t *h);

/* 0: the default arithmetic (carried heading vector, fused transit); 1: the reference's operation order
 * (BN_FLAG_REFERENCE_ORDER, or selected because dt * max|omega| > 0.5).  Kernel launches one solve costs: 1 or 2. */
int32_t bn_mppi_arithmetic(const bn_mppi_t *h);
int32_t bn_mppi_launches_per_solve(const bn_mppi_t *h);
/* Kernel launches of one bn_mppi_forward_async / bn_mppi_forward_state_async / bn_mppi_solve call (solve AND its tail): 1 on the
 * latency kernel (see bn_mppi_forward_state_async), else 2. */
int32_t bn_mppi_launches_per_forward(const bn_mppi_t *h);
/* How the cell index divides by the resolution (grid_map.py:203): 2 = exact multiplication (power-of-two resolution), 1 = the
 * three-instruction correctly rounded quotient, validated exhaustively on the device at create for this resolution and these limits
 * (bn_mppi_create refuses a resolution that fails the check; none is known). */
int32_t bn_mppi_fast_quotient(const bn_mppi_t *h);

/* With BN_FLAG_PROFILE: mean duration in milliseconds of the rollout kernel and of
 * the finish kernel over the solves since the last call (HIP events on the
 * handle's stream), and how many solves that covers.  Synchronises.
 * Two-launch mode: an event pair around every kernel.  Pipelined mode (one ~15 us
 * launch per solve, back to back): one event per group of 10 launches, mean = group
 * time / 10 (an event pair per launch would add its own dispatch latency);
 * finish_ms is 0 there -- the tail rides inside the next launch. */
int bn_mppi_kernel_ms(bn_mppi_t *h, float *rollout_ms, float *finish_ms, int32_t *n_solves);

/* Algorithmic HBM bytes of one solve in the current mode (DESIGN.md "Roofline"). */
int64_t bn_mppi_algorithmic_bytes(const bn_mppi_t *h, bn_noise_kind noise);
/* ... with the map term (4 G^2) replaced by the reachable window the kernels stage (4 WN^2): the bytes a solve has to move when
 * only a corner of the map can be reached within the horizon.  The roofline fraction of a lean launch against THIS figure is the
 * honest one (SURVEY 8d's lean formula counts the whole map). */
int64_t bn_mppi_algorithmic_bytes_window(const bn_mppi_t *h, bn_noise_kind noise);

/*
 * TraversabilityModel._infer_risk_map, traversability_model.py:28-51 (runs once per dynamics object, in
 * UnicycleModel.__init__): the (G,G) risk map from the predicted slip distribution Normal(mean, std).
 *   BN_RISK_EXPECTED  mean                                             (:30-31)
 *   BN_RISK_VAR       torch.quantile(samples, confidence, dim=0)       (:33-36), linear interpolation: exact selection of the
 *                     two ranks and at::lerp's FUSED form (fma(w, b - a, a) for |w| < 0.5, else fma(w - 1, b - a, b)): equal
 *                     to torch.quantile by value on the same samples.  A NaN or +-inf mean, or a NaN std, gives NaN.
 *   BN_RISK_CVAR      nanmean of the samples strictly above that       (:37-42)
 * samples_i = mean + std * z_i; z = (num_samples, G, G) standard normals supplied by the caller (the
 * reference's Normal.sample stream, for parity) or NULL: generated in the kernel (Philox, keyed by seed).
 * Stateless; host-resident arguments are copied and the call synchronises, device-resident ones are only
 * enqueued on `stream`.  Errors: bn_risk_last_error().
 */
typedef enum bn_risk_metric { BN_RISK_EXPECTED = 0, BN_RISK_VAR = 1, BN_RISK_CVAR = 2 } bn_risk_metric;
int bn_risk_map_infer(int32_t device_id, void *stream, const float *mean, const float *std, bn_mem_kind where_in,
                      int32_t grid_size, bn_risk_metric metric, float confidence, int32_t num_samples,
                      const float *z, bn_mem_kind where_z, uint64_t seed, float *out, bn_mem_kind where_out);
const char *bn_risk_last_error(void);
/*
 * The benchmark's form: num_maps maps under num_settings (metric, confidence) pairs in ONE launch on `stream`.  Device pointers
 * only: mean, std (num_maps, G, G); z (num_maps, num_samples, G, G) or NULL; seeds (num_maps) or NULL (every seed 0); out
 * (num_settings, num_maps, G, G).  metrics and confidences are host arrays, read before the call returns.  A wave draws its
 * cell's samples once -- the Philox counters are bn_risk_map_infer's: the cell index within the map, the lane block, the map's
 * seed -- and evaluates every setting on them, so out[c][m] is bit for bit what bn_risk_map_infer returns for (mean[m], std[m],
 * metrics[c], confidences[c], num_samples, z[m] or seeds[m]).  num_settings in [1, BN_RISK_MAX_SETTINGS]; num_samples in
 * [2, 4096] and confidences in [0, 1] wherever a setting samples.  Nothing synchronises.  Errors: bn_risk_last_error().
 */
#define BN_RISK_MAX_SETTINGS 16
int bn_risk_maps_infer(int32_t device_id, void *stream, const float *mean_device, const float *std_device, int32_t num_maps,
                       int32_t grid_size, const bn_risk_metric *metrics, const float *confidences, int32_t num_settings,
                       int32_t num_samples, const float *z_device, const uint64_t *seeds_device, float *out_device);

/*
 * An episode log reduced to its outcome on the device (csrc/score_kernels.hip): what the benchmark reports per episode.  Device
 * pointers only, one launch on `stream`, nothing synchronises.  Errors: bn_score_last_error().
 *   states (n_steps + 1, B, 3), rewards (n_steps, B), goals (B, 2)
 *   end_step (B)   how many leading rows count, clamped to [0, n_steps]; NULL: done_step + 1 where the goal was reached, else n_steps
 *   done_step (B)  the 0-based index of the step whose resulting state first lay within the goal threshold, or -1: the word
 *                  bn_mppi_episode_async and bn_astar_dwa_episode_async write (from bn_clrrt_loop_log: done_iter where the
 *                  status is BN_CL_GOAL, else -1)
 *   stopped (B) or NULL: non-zero = the planner gave up (a bn_astar_dwa_status, a CL-RRT status that is no goal and no time limit)
 *   invalid (B) or NULL: non-zero = the start or the goal was not traversable
 * A row whose reward is NaN is no step (the frozen rows of the A* + DWA log, the replan rows of the CL-RRT log): it adds nothing,
 * but its state is still the rover's position.  Outputs, (B) each:
 *   outcome         bn_episode_outcome: invalid wins, then done_step >= 0, then stopped, else the time limit
 *   steps           counted rows;  time: `steps` successive += delta_t in float64 (PlanetaryEnv._elapsed_time)
 *   path_length     float64 sum, in step order, of the float64 distances between consecutive positions over the counted rows
 *   reward_sum      float64;  reward_min float32, NaN when steps == 0
 *   stuck_steps     counted rows with reward <= stuck_threshold, compared in float32
 *   final_distance  float64, from the state after the last row inside end_step to the goal
 */
typedef enum bn_episode_outcome { BN_OUTCOME_GOAL = 0, BN_OUTCOME_TIME_LIMIT = 1, BN_OUTCOME_STOPPED = 2, BN_OUTCOME_INVALID = 3 } bn_episode_outcome;
int bn_episode_score(int32_t device_id, void *stream, const float *states_device, const float *rewards_device, const float *goals_device,
                     const int32_t *end_step_device, const int32_t *done_step_device, const int32_t *stopped_device,
                     const uint8_t *invalid_device, int32_t n_steps, int32_t num_episodes, float stuck_threshold, double delta_t,
                     int32_t *outcome_device, int32_t *steps_device, double *time_device, double *path_length_device,
                     double *reward_sum_device, float *reward_min_device, int32_t *stuck_steps_device, double *final_distance_device);
const char *bn_score_last_error(void);

/*
 * The model-evaluation stage (csrc/eval_kernels.hip): three reductions over num_maps maps of `cells` cells each,
 * on arrays that already sit on the device.  Device pointers only, everything is enqueued on `stream`, nothing synchronises, the
 * outputs are overwritten (only `total` of bn_eval_slip_async is added to).  num_classes in [1, BN_EVAL_MAX_CLASSES].  Every
 * function refuses a null pointer, num_maps < 1, cells < 1 and a count out of its range with BN_ERR_INVALID before it touches the
 * device.  Errors: bn_eval_last_error().
 *
 * bn_eval_confusion_async: true_classes, pred_classes (num_maps, cells) int32.
 *   table (num_maps, C, C)   cells with true class t and predicted class p, at [t][p]
 *   ignored (num_maps)       cells with either class outside [0, C): they are in no table entry
 *
 * bn_eval_slip_async: the predicted slip N(mean, std^2) against the latent N(latent_mean, latent_std^2) and, with slips (may be
 * NULL), against one observation y per cell; all (num_maps, cells) float32, classes int32.  A cell belongs to the group (true
 * class c, slope bin j), j = min(max(trunc((double)slope * num_bins / max_slope), 0), num_bins - 1) in float64: num_bins equal
 * bins over [0, max_slope], closed on the left, a slope below 0 in the first and one at or above max_slope in the last.
 * num_bins in [1, BN_EVAL_MAX_BINS] with C * num_bins <= BN_EVAL_MAX_GROUPS; max_slope > 0.  With d = mean - latent_mean,
 * e = y - mean, all in float64 on the float32 inputs:
 *   sums (num_maps, C, num_bins, BN_EVAL_SLIP_SUMS) per map and group, in this order:
 *       sum d, sum |d|, sum d^2, sum std, sum latent_std,
 *       sum KL(latent || predicted) = (log(std / latent_std) + (latent_std^2 + d^2) / (2 std^2)) - 0.5,
 *       sum NLL = 0.5 log(2 pi std^2) + e^2 / (2 std^2), sum (e / std)^2     (both 0 without slips)
 *   counts (num_maps, C, num_bins, 2)  the group's cells, and those of them with |e| <= 2 std (0 without slips)
 *   invalid (num_maps)   cells in no sum and no count: a class outside [0, C), a non-finite slope, mean, std, latent_mean,
 *                        latent_std or y, std <= 0 or latent_std <= 0 (a class without a regressor predicts std = 0)
 *   total (C, num_bins, BN_EVAL_SLIP_SUMS) or NULL: in/out, the maps' `sums` are added onto it in map order, so that calls over
 *                        successive runs of maps leave the bits of one call over all of them
 * The float64 sums are added in a fixed order that depends on the cell index and the map index alone: not on
 * num_maps, the grid or atomics; a map's entries are bit for bit the same in any batch.  workspace: at least
 * bn_eval_slip_workspace_bytes(...) bytes (0 for arguments out of range), free again once the stream has passed the call.
 *
 * bn_eval_risk_async: risk (num_settings, num_maps, cells) float32, the tensor bn_risk_maps_infer writes; slips y and classes
 * (num_maps, cells); num_settings in [1, BN_RISK_MAX_SETTINGS].  stuck(v) = 1.0f - clamp(v, 0, 1) <= stuck_threshold in float32,
 * the environment step's arithmetic.  One launch handles every setting and reads y and the classes once.
 *   counts (num_maps, num_settings, C, BN_EVAL_RISK_COUNTS) per map, setting k and true class:
 *       [0] y > risk_k;  [1 + 2 stuck(risk_k) + stuck(y)]: [1] believed safe and safe, [2] BELIEVED SAFE, ACTUALLY STUCK,
 *       [3] believed stuck, actually safe, [4] believed stuck and stuck
 *   invalid (num_maps, num_settings)  cells in no count: a class outside [0, C), a non-finite y or a non-finite risk_k
 */
#define BN_EVAL_MAX_CLASSES 64
#define BN_EVAL_MAX_BINS 64
#define BN_EVAL_MAX_GROUPS 512
#define BN_EVAL_SLAB_CELLS 4096
#define BN_EVAL_SLIP_SUMS 8
#define BN_EVAL_RISK_COUNTS 5
int bn_eval_confusion_async(int32_t device_id, void *stream, const int32_t *true_classes_device, const int32_t *pred_classes_device,
                            int32_t num_maps, int64_t cells, int32_t num_classes, int64_t *table_device, int64_t *ignored_device);
size_t bn_eval_slip_workspace_bytes(int32_t num_maps, int64_t cells, int32_t num_classes, int32_t num_bins);
int bn_eval_slip_async(int32_t device_id, void *stream, const float *mean_device, const float *std_device, const float *latent_mean_device,
                       const float *latent_std_device, const float *slopes_device, const int32_t *classes_device, const float *slips_device,
                       int32_t num_maps, int64_t cells, int32_t num_classes, int32_t num_bins, double max_slope, double *sums_device,
                       int64_t *counts_device, int64_t *invalid_device, double *total_device, void *workspace_device, size_t workspace_bytes);
int bn_eval_risk_async(int32_t device_id, void *stream, const float *risk_device, const float *slips_device, const int32_t *classes_device,
                       int32_t num_settings, int32_t num_maps, int64_t cells, int32_t num_classes, float stuck_threshold,
                       int64_t *counts_device, int64_t *invalid_device);
const char *bn_eval_last_error(void);

/*
 * The task stage (csrc/task_kernels.hip): the truly passable ground of num_maps maps of H x W cells, its connected
 * regions, and start/goal pairs drawn inside one region.  Device pointers only, everything is enqueued on `stream`, nothing
 * synchronises or allocates, the outputs are overwritten.  H, W in [1, BN_TASK_MAX_SIDE] with H * W <= BN_TASK_MAX_CELLS, num_maps
 * in [1, BN_TASK_MAX_MAPS].  Every function checks every argument before it touches the device (BN_ERR_INVALID).  Every result is
 * an integer or a fixed function of integers.  Errors: bn_task_last_error().
 *
 * bn_task_mask_async: mean, std (num_maps, cells) float32, the latent slip model.  In float32, a rounded product then a rounded sum:
 *   mask (num_maps, cells) uint8 = isfinite(mean) && isfinite(std) && 1.0f - clamp(mean + kappa * std, 0, 1) > stuck_threshold
 * the complement of the environment step's stuck rule at the slip mean + kappa std; kappa = 0 reads the mean.
 *
 * bn_task_label_async: mask (num_maps, H, W) uint8, non-zero = passable (bn_task_mask_async's, or the caller's own);
 * connectivity 4 or 8.
 *   labels (num_maps, H, W) int32   the smallest linear index iy * W + ix of the cell's component, -1 on a blocked cell
 *   sizes (num_maps, H * W) int32   the component's cell count at such a smallest index, 0 elsewhere
 *   stats (num_maps, BN_TASK_STATS) int32: passable cells, components, the largest size, the label of the largest (the smallest
 *          label wins a tie; -1 without a component), error flags (BN_TASK_ERR_*: a loop reached its bound, the map's labels are
 *          not to be used), three zeros
 * The labelling is unique: a map's outputs depend neither on the order workgroups run in nor on the batch it is in.  workspace:
 * at least bn_task_workspace_bytes(num_maps, H, W) bytes (0 for a shape out of range), free once the stream has passed the call.
 *
 * bn_task_sample_async: labels and sizes as bn_task_label_async wrote them.  Attempt a of pair p of map m draws
 *   r = philox4x32_10(counter {a, p, first_map + m, 0x5441534B}, key {lo32(seed), hi32(seed)});
 * with Win = W - 2 border, Hin = H - 2 border, n = Win Hin the start cell is s = mulhi32(r0, n): (s % Win + border, s / Win + border),
 * the goal cell likewise from r1.  An attempt is accepted when both cells are labelled >= 0 with one label, sizes[label] >=
 * min_component_cells and dx^2 + dy^2 >= min_separation_sq in integer cells; a pair takes the lowest accepted a < max_attempts
 * (a multiple of 64 in [64, BN_TASK_MAX_ATTEMPTS]).  2 * border < min(H, W); num_pairs in [1, BN_TASK_MAX_PAIRS].
 *   cells (num_maps, num_pairs, 4) int32     (sx, sy, gx, gy), all -1 when no attempt is accepted
 *   attempt (num_maps, num_pairs) int32      the accepted attempt, -1 when none
 *   positions (num_maps, num_pairs, 4) float32   the cell centres fl32(x0 + fl32(fl32(i + 0.5) * resolution)), NaN when none
 */
#define BN_TASK_TILE 32
#define BN_TASK_STATS 8
#define BN_TASK_MAX_SIDE 4096
#define BN_TASK_MAX_CELLS (1 << 24)
#define BN_TASK_MAX_MAPS 4096
#define BN_TASK_MAX_PAIRS 65536
#define BN_TASK_MAX_ATTEMPTS 4096
#define BN_TASK_ERR_TILE 1
#define BN_TASK_ERR_UNITE 2
#define BN_TASK_ERR_FLATTEN 4
size_t bn_task_workspace_bytes(int32_t num_maps, int32_t H, int32_t W);
int bn_task_mask_async(int32_t device_id, void *stream, const float *mean_device, const float *std_device, int32_t num_maps, int64_t cells,
                       float kappa, float stuck_threshold, uint8_t *mask_device);
int bn_task_label_async(int32_t device_id, void *stream, const uint8_t *mask_device, int32_t num_maps, int32_t H, int32_t W,
                        int32_t connectivity, int32_t *labels_device, int32_t *sizes_device, int32_t *stats_device, void *workspace_device,
                        size_t workspace_bytes);
int bn_task_sample_async(int32_t device_id, void *stream, const int32_t *labels_device, const int32_t *sizes_device, int32_t num_maps,
                         int32_t H, int32_t W, int32_t num_pairs, uint64_t seed, int64_t first_map, int32_t border, int64_t min_separation_sq,
                         int32_t min_component_cells, int32_t max_attempts, float x0, float y0, float resolution, int32_t *cells_device,
                         int32_t *attempt_device, float *positions_device);
const char *bn_task_last_error(void);

/*
 * AStar (src/planners/global_planners/search_based/astar.py), the A* global planner, as one goal-rooted shortest-path solve
 * per (map, goal) on the GPU: the cost-to-go field D and a one-byte next-hop map for B instances of one H x W shape, then
 * O(path length) host walks per start (csrc/astar_kernels.hip).  Graph and arithmetic are astar.py's: 8-connected cells
 * (ix, iy) indexed [iy, ix], edges into cells with risk > stuck_threshold (NaN risk too), weight
 * sqrt_f32(f32(dx^2 + dy^2) + dz * dz).  Errors: bn_astar_last_error().
 */
typedef struct bn_astar bn_astar_t;
/* astar.py:33-71 (constructor buffers). */
int bn_astar_create(int32_t device_id, int32_t H, int32_t W, int32_t B, bn_astar_t **out);
void bn_astar_destroy(bn_astar_t *h);
/* astar.py:53-58: heights and risks (H, W), the stuck threshold and the map resolution (shared by every instance). */
int bn_astar_set_map(bn_astar_t *h, int32_t inst, const float *heights, const float *risks, bn_mem_kind where,
                     float stuck_threshold, double resolution);
/* astar.py:71: the goal cell; an out-of-bounds or collision goal is accepted (every path is then none, 0). */
int bn_astar_set_goal(bn_astar_t *h, int32_t inst, int32_t ix, int32_t iy);
/* astar.py:96-122 for every start at once: field + next-hop map on `stream`, then an async copy of next to pinned memory. */
int bn_astar_solve_async(bn_astar_t *h, void *stream);
/* Waits for the last solve; BN_ERR_STATE if its kernel reported a failure. */
int bn_astar_sync(bn_astar_t *h);
/* Device time of the last solve's kernels in ms. */
int bn_astar_kernel_ms(bn_astar_t *h, float *ms);
/* astar.py:73-122 + _reconstruct_path :194-213: nodes (ix, iy) from the start to the goal into out_xy (2 * max_len int32).
 * Returns the node count, 0 if the goal is unreachable (None), BN_ERR_INVALID for a start out of bounds. */
int bn_astar_path(bn_astar_t *h, int32_t inst, int32_t ix, int32_t iy, int32_t *out_xy, int32_t max_len);
/* Test hook: device pointers of instance inst's D (H*W float32) and next (H*W uint8: 0-7 direction in astar.py:154-163
 * order, 8 goal, 255 unreachable). */
int bn_astar_buffers(bn_astar_t *h, int32_t inst, void **D_dev, void **next_dev);
/*
 * Jump tables behind the latest solve (csrc/astar_kernels.hip), per instance: hops (H*W int32), the number of hops along next to
 * the goal (0 at the goal, -1 where the walk ends on an unreachable cell: everywhere for a goal out of bounds or in collision),
 * and jump (levels, H*W) int32, jump[k][c] = the cell (iy * W + ix) reached from c after 2^k hops (the goal and unreachable cells
 * map to themselves), levels = max(1, ceil(log2(H*W))): every node index of a path is a sum of kept powers of two.  Footprint
 * B * (levels + 2) * H*W * 4 bytes (the levels and two hop buffers), allocated by the first build.  The build is levels + 1
 * launches on `stream` behind the solve, whatever the map holds.  It validates next: a code in 9-254, a hop off the map, or a
 * cycle (a walk still stepping after 2^levels hops) sets the tables' error word, reported as BN_ERR_STATE by bn_astar_sync and by
 * every consumer, with the first offending cell in the message.  bn_astar_set_map, bn_astar_set_goal and bn_astar_solve_async
 * make the tables stale: consumers then return BN_ERR_STATE.
 */
int bn_astar_jump_build_async(bn_astar_t *h, void *stream);
/* Device time of the last table build in ms. */
int bn_astar_jump_ms(bn_astar_t *h, float *ms);
/* Paths for n start cells of instance inst from the tables, on the device: starts_xy (n, 2) int32 (ix, iy), host or device;
 * out_len_device (n) int32: the node count of the path, goal included (bn_astar_path's return value), 0 where the goal is
 * unreachable, -1 for a start out of bounds; out_xy_device (n, max_len, 2) int32: the first min(len, max_len) nodes of each row,
 * the rest -1 (may be NULL with max_len = 0).  Waits on the host for a pending table build (its validation); the paths
 * themselves are enqueued on `stream`.  Starts on the host (BN_MEM_HOST) go through one staging buffer per handle: the call
 * then also waits on the host for earlier readers of the handle and for the copy on `stream`, so it is synchronous up to the
 * paths kernel; pass the starts on the device to keep the call asynchronous.  n = 0 is a no-op. */
int bn_astar_paths_async(bn_astar_t *h, int32_t inst, const int32_t *starts_xy, bn_mem_kind where, int32_t n, int32_t max_len,
                         int32_t *out_xy_device, int32_t *out_len_device, void *stream);
/* Test hook: device pointers of instance inst's hops (H*W) and jump (levels, H*W), the level count and the element size. */
int bn_astar_jump_buffers(bn_astar_t *h, int32_t inst, void **hops_dev, void **jump_dev, int32_t *levels, int32_t *elem_bytes);
const char *bn_astar_last_error(void);

/*
 * The A* + DWA closed loop of test_astar_dwa.py:179-211 on the device for the B instances of h (csrc/astar_dwa.hip), one
 * workgroup per instance, no host round trip: per control step the A* path from the current cell (astar.py:73-122 as a walk of
 * a's solved next-hop map), DWA.forward (dwa.py:116-153) and PlanetaryEnv.step (planetary_env.py:189-219).
 *   start cell  int((x - x_limits[0]) / res) in f32, truncated (AStar._pos_to_index).  A start out of bounds, a goal out of
 *               bounds or in collision (astar.py:88-94) freezes the instance with a status and the step (the reference raises).
 *   path        point = (f32(ix) * f32(res), f32(iy) * f32(res)), start cell included.  An unreachable start is the reference's
 *               None: DWA keeps the previous path, the walk from the instance's root cell (the last start whose walk reached
 *               the goal); no root cell yet: the stage cost runs against the goal (dwa.py:243-247).
 *   env step    observation-mode transit with the slip draw of episode step j: z_device row j of this call, or Philox keyed by
 *               (env seed, j) as bn_mppi_env_step(..., step_index = j); honours bn_mppi_env_set_freeze.
 * Steps are counted from bn_astar_dwa_reset; the root cells, the step count and the statuses persist across calls until then,
 * the window centre in the caller's prev_action_device: episode(n) == episode(k) then episode(n - k), bit for bit.
 */
typedef enum bn_astar_dwa_status {
    BN_AD_OK = 0,               /* running                                                                  */
    BN_AD_OUT_OF_BOUNDS = 1,    /* ValueError("Start or goal position is out of bounds.") (astar.py:88-92)  */
    BN_AD_GOAL_COLLISION = 2,   /* ValueError("Goal position is not traversable.") (astar.py:93-94)         */
    BN_AD_FIELD_ERROR = 3       /* the A* solve failed, or a next-hop walk broke (not a valid field)        */
} bn_astar_dwa_status;
/* n_steps control steps on h's stream, ordered behind a's latest bn_astar_solve_async by an event.  Needs bn_mppi_env_attach and
 * the goals of h; a on h's device with h's B and H = W = grid_size; num_lin_vel * num_ang_vel <= 1024.  states0 (B,3) the
 * current environment states; prev_action_device (B,2) in/out; z_device (n_steps, B) or NULL. */
int bn_astar_dwa_episode_async(bn_mppi_t *h, bn_astar_t *a, int32_t n_steps, const float *states0, bn_mem_kind where,
                               float *prev_action_device, const float a_lim[2], float dwa_delta_t, int32_t num_lin_vel,
                               int32_t num_ang_vel, float lookahead, const float *z_device);
/* The latest call's log (any pointer may be NULL): states (n+1,B,3) with [0] the call's start, rewards (n,B), actions (n,B,2),
 * sub_goals (n,B,2) (the stage-cost target); a frozen instance's rows keep its state and hold NaN elsewhere.  done_step (B): first
 * episode step whose resulting state is within the goal threshold, or -1; status (B) bn_astar_dwa_status; status_step (B): the
 * episode step at which it was set.  BN_ERR_STATE if a walk broke (the kernel's error word). */
int bn_astar_dwa_episode_log(bn_mppi_t *h, float *states, float *rewards, float *actions, float *sub_goals,
                             int32_t *done_step, int32_t *status, int32_t *status_step);
/* Device views of the latest call's log (bn_episode_score): states (n_steps + 1, B, 3) and rewards (n_steps, B) as the leading rows
 * of buffers laid out for row_capacity steps, done_step (B) and status (B), both counted from the last reset.  Valid until the next
 * call; any pointer may be NULL.  Nothing is copied, and the error word is not read (bn_astar_dwa_episode_log does that). */
int bn_astar_dwa_episode_buffers(bn_mppi_t *h, const float **states_device, const float **rewards_device,
                                 const int32_t **done_step_device, const int32_t **status_device, int32_t *n_steps, int32_t *row_capacity);
/* Forget the root cells, the statuses and the step count: a new episode, or a new A* solve. */
int bn_astar_dwa_reset(bn_mppi_t *h);
/* Set instance b's root cell (ix, iy), or forget it with ix < 0: starts a teacher-forced step from a given previous path. */
int bn_astar_dwa_set_root(bn_mppi_t *h, int32_t instance, int32_t ix, int32_t iy);
/* How the episode reads the path: 0 (default) one lane walks next node by node; 1 every lane fetches its own node through a's
 * jump tables (bn_astar_jump_build_async), the same nodes in the same order, so every output is bit-identical.  With 1,
 * bn_astar_dwa_episode_async returns BN_ERR_STATE unless a's tables are current, and the tables' error word freezes the
 * instances with BN_AD_FIELD_ERROR as the field's does. */
int bn_astar_dwa_set_walk(bn_mppi_t *h, int32_t mode);

/*
 * Terrain generation (csrc/terrain_kernels.hip): TerrainGeometry.set_terrain_geometry (craters, fBm, Horn slopes) and
 * TerrainTraversability.set_traversability (src/environments/terrain_properties.py) for B instances of one grid size G per
 * launch.  The random draws are either made on the host in the reference's order (benchnav_amd/terrain.py) and set here
 * (bn_terrain_set_draws), or made on the device from the seeds (bn_terrain_set_draw_params + bn_terrain_draw_async: the same
 * MT19937 stream); the device does the arithmetic.  Outputs are (B, G, G) float32: heights, slopes (degrees), latent slip mean and stddev.  G <= 1024.
 * Host arguments are copied synchronously.  Errors: bn_terrain_last_error().
 */
typedef struct bn_terrain bn_terrain_t;
int bn_terrain_create(int32_t device_id, int32_t G, int32_t B, bn_terrain_t **out);
void bn_terrain_destroy(bn_terrain_t *h);
/* The grid map's resolution, TerrainGeometry's roughness_exponent and amplitude_gain, and is_fractal. */
int bn_terrain_set_geometry(bn_terrain_t *h, double resolution, double roughness_exponent, double amplitude_gain, int32_t is_fractal);
/* The draws of every instance: phases (B, nph) float32 uniforms of the fBm spectrum, nph = (G'/2 + 1)^2 + (G'/2 - 1)^2 with
 * G' = G + 2; crater_count (B); per crater, in placement order, crater_int (B, max_craters, 8) = sx, sy, ex, ey (the padded-grid
 * slice [sy:ey, sx:ex]), psx, psy (the profile's offset in the slice), n (profile points per axis), lin offset, and crater_val
 * (B, max_craters, 2) = float32 radius and -tan(deg2rad(angle)); lin (lin_len) holds each crater's linspace(-r, r, n). */
int bn_terrain_set_draws(bn_terrain_t *h, const float *phases, const int32_t *crater_count, const int32_t *crater_int,
                         const float *crater_val, int32_t max_craters, const float *lin, int64_t lin_len);
/* The parameters of the draws made on the device (set_terrain_geometry's, and create_shading's thresholds): is_crater, num_craters
 * (at most 64, the crater slots of the device draws), crater_margin, the angle range in degrees and the radius range (> 0) in
 * metres; with_light != 0 also draws the light source of the colouring between lower_threshold and upper_threshold.  Needs the
 * geometry (the resolution sizes the profile slots: B x num_craters x (2 max_radius / resolution + 2) values, at most 2^30). */
int bn_terrain_set_draw_params(bn_terrain_t *h, int32_t is_crater, int32_t num_craters, double crater_margin, double min_angle,
                               double max_angle, double min_radius, double max_radius, int32_t with_light, double lower_threshold,
                               double upper_threshold);
/* Enqueues the draws of B instances on `stream` from seeds (B, host; the low 32 bits seed MT19937 as torch's CPU generator does):
 * the crater loop, the crater tables, the phases and, with with_light, the light vectors (bn_terrain_set_coloring comes first and
 * its `light` is then replaced).  Writes what bn_terrain_set_draws would upload, so it counts as "draws set" for
 * bn_terrain_generate_async on the same stream. */
int bn_terrain_draw_async(bn_terrain_t *h, const uint64_t *seeds, void *stream);
/* The sizes bn_terrain_read_draws' tables have under the draw parameters as they stand: S crater slots per instance and the
 * profile stride of a slot. */
int bn_terrain_draw_layout(bn_terrain_t *h, int32_t *slots, int32_t *stride);
/* Waits and copies what the device drew (any pointer may be NULL): records (B, 4) int32 = attempts, gave_up, status (0, or 1 + the
 * first crater whose slices disagree in shape: it was not carved), craters placed; centers (B, S, 2) float32, angles (B, S) float64
 * degrees, S slots (bn_terrain_draw_layout); light_uniforms (B, 2) and light (B, 3) float32; crater_int (B, S, 8) and crater_val
 * (B, S, 2) as in bn_terrain_set_draws, the lin offset being slot * stride (-1 for a crater that
 * does not fit); lin (B, S, stride) float32; phases (B, nph) float32. */
int bn_terrain_read_draws(bn_terrain_t *h, int32_t *records, float *centers, double *angles, float *light_uniforms, float *light,
                          int32_t *crater_int, float *crater_val, float *lin, float *phases);
/* Class maps t_classes (B, G, G) and per-class rows of 6 float32: present (0: the class has no model, its cells stay inf),
 * f32(slip_sensitivity * 1e-3), slip_nonlinearity, slip_offset, base_noise_scale, slope_noise_scale.  t_classes may be NULL: the
 * device's class map is left as it is (the colouring step writes it, bn_terrain_set_coloring). */
int bn_terrain_set_slip(bn_terrain_t *h, const int32_t *t_classes, const float *class_params, int32_t num_classes);
/* Enqueues the whole generation on `stream`. */
int bn_terrain_generate_async(bn_terrain_t *h, void *stream);
/* Waits for the last generation. */
int bn_terrain_sync(bn_terrain_t *h);
/* Device pointers of the outputs, (B, G, G) float32 each; valid after the generation on its stream. */
int bn_terrain_buffers(bn_terrain_t *h, void **heights, void **slopes, void **mean, void **stddev);
/* Waits and copies the outputs to host memory (any pointer may be NULL). */
int bn_terrain_copy_out(bn_terrain_t *h, float *heights, float *slopes, float *mean, float *stddev);
/* TerrainColoring.set_terrain_class_coloring (terrain_properties.py:364-523) as part of the generation.  enable = 0 switches it off
 * again (every other argument is ignored).  thresholds (B, C) float32 = cumsum(occupancy) * 100 and start (B) = the first class
 * with occupancy > 0 (generate_multi_terrain :428-431); color_table (C, 3) float32, row i the colour of class i (create_color_map
 * :462-470); light (B, 3) float32 light vectors and ambient_intensity (create_shading :511-521); C <= 64.  The noise field of :418-420
 * is either `noise` (B, G, G) float32, or, with noise = NULL, the library's own gradient noise at (x, y) / feature_size keyed by
 * seeds (B).  The generation then writes the class map ahead of the slip maps and the colours after them, and counts
 * per instance the cells left without a class and the cells whose class is >= num_slip_models. */
int bn_terrain_set_coloring(bn_terrain_t *h, int32_t enable, const float *thresholds, const int32_t *start, int32_t num_classes,
                            const float *color_table, const float *light, float ambient_intensity, float feature_size,
                            const float *noise, const uint64_t *seeds, int32_t num_slip_models);
/* create_color_map + create_shading (:462-523) on the caller's heights (B, G, G) float32 and classes (B, G, G) int32, host
 * pointers: enqueues the colour kernel on `stream`; the result is the colours buffer of bn_terrain_color_buffers.  A class below 0
 * takes row 0 of the table, one above C - 1 row C - 1 (the colour map's under and over entries). */
int bn_terrain_colorize(bn_terrain_t *h, const float *heights, const int32_t *t_classes, const float *color_table, int32_t num_classes,
                        const float *light, float ambient_intensity, void *stream);
/* Device pointers: classes (B, G, G) int32, colours (B, 3, G, G) float32, the raw noise field (B, G, G) float32. */
int bn_terrain_color_buffers(bn_terrain_t *h, void **classes, void **colors, void **noise);
/* Waits for the last coloured generation; per instance, the cells with class -1 (the warning of :440-441) and the cells whose
 * class has no slip model (set_traversability's ValueError, :554-557). */
int bn_terrain_class_counts(bn_terrain_t *h, int32_t *unassigned, int32_t *beyond);
/* Test hook: instance inst's scaled fBm spectrum (G', G') complex64 as interleaved float32 pairs. */
int bn_terrain_spectrum(bn_terrain_t *h, int32_t inst, float *out);
const char *bn_terrain_last_error(void);

/* ------------------------------------------------------------------------------------------------------------------------------
 * The RRT global planner (csrc/rrt_kernels.hip): `RRT` and `Tree` of src/planners/global_planners/sampling_based/{rrt,tree}.py for
 * B planners that share limits and parameters, one workgroup each, bit for bit with the reference's CPU run:
 * torch's MT19937 stream of each instance's seed parsed into samples, the tree grown by nearest neighbour + steer, then the goal
 * test, the pick (lowest cost, then lowest index among the near-goal nodes) and the path.  Errors: the rrt error string below.
 * ---------------------------------------------------------------------------------------------------------------------------- */
typedef enum bn_rrt_flags {
    BN_RRT_FLAG_GLOBAL_NODES = 1,  /* keep the nodes in global memory at any size (the path taken above 8191 iterations) */
    BN_RRT_FLAG_ONE_WAVE = 2,      /* grow with one wave per instance (the slower of the two, DESIGN.md 4.6: kept for measurements) */
    BN_RRT_FLAG_FOUR_WAVES = 4     /* grow with 256 threads per instance (the default) */
} bn_rrt_flags;

typedef enum bn_rrt_buffer_id {
    BN_RRT_BUF_NODES = 0,          /* (B, max_iterations + 1, 2) float32 */
    BN_RRT_BUF_EDGES = 1,          /* (B, max_iterations + 1) int32, the parent; -1 at the root */
    BN_RRT_BUF_COSTS = 2,          /* (B, max_iterations + 1) float32 */
    BN_RRT_BUF_COUNTS = 3,         /* (B) int32 nodes in the tree */
    BN_RRT_BUF_SAMPLES = 4,        /* (B, max_iterations, 2) float32: the sample of every iteration */
    BN_RRT_BUF_SAMPLE_FLAGS = 5,   /* (B, max_iterations) int32: 1 where the sample is the goal */
    BN_RRT_BUF_PATHS = 6,          /* (B, path_cap, 2) float32, root first, NaN beyond the path */
    BN_RRT_BUF_RESULTS = 7         /* (B, 4) int32: found, picked node (-1), path length, near-goal nodes */
} bn_rrt_buffer_id;

typedef struct bn_rrt_config {
    uint32_t struct_size;          /* sizeof(bn_rrt_config), set by the init function */
    int32_t device_id;
    int32_t num_instances;         /* B */
    int32_t max_iterations;        /* rrt.py:34; every iteration adds a node (_steer always returns feasible) */
    int32_t path_cap;              /* rows of the path buffer per instance; 0 = max_iterations + 1 (no path is longer) */
    uint32_t flags;                /* bn_rrt_flags */
    double x_limits[2], y_limits[2];
    double delta_distance;         /* rrt.py:35 */
    double goal_sample_rate;       /* rrt.py:36 */
    double goal_threshold;         /* _is_goal_reached's 0.1 */
    uint64_t seed;                 /* 0 ... 2^32 - 1: the stream every instance starts from when the first plan passes no seeds */
} bn_rrt_config;

typedef struct bn_rrt bn_rrt_t;
void bn_rrt_config_init(bn_rrt_config *cfg);
/* Arguments are checked before the device is touched; without a device BN_ERR_NO_DEVICE ("no CPU fallback"). */
int bn_rrt_create(const bn_rrt_config *cfg, bn_rrt_t **out);
void bn_rrt_destroy(bn_rrt_t *h);
/* One forward() of every instance on `stream`: starts and goals are HOST (B, 2) float32 (consumed before the call returns; a
 * position out of the limits is BN_ERR_INVALID and nothing is launched).  seeds: HOST (B) uint64, each 0 ... 2^32 - 1, reseeds the
 * streams as constructing the planner does; NULL continues every stream where its last plan left it (the reference does not
 * reseed between forward() calls). */
int bn_rrt_plan_async(bn_rrt_t *h, void *stream, const float *starts, const float *goals, const uint64_t *seeds);
/* The growth, the goal test and the path on the caller's samples (B, max_iterations, 2) float32, `where` a bn_mem_kind, in place
 * of the stream's (which is left where it is). */
int bn_rrt_grow_from_samples_async(bn_rrt_t *h, void *stream, const float *starts, const float *goals, const void *samples, int where);
int bn_rrt_sync(bn_rrt_t *h);
/* Device pointer and size in bytes of one of the handle's buffers (bn_rrt_buffer_id); valid until the handle is destroyed. */
int bn_rrt_device_buffer(bn_rrt_t *h, int which, void **ptr, size_t *bytes);
/* Where the growth kernel keeps the tree: 0 = global memory, 1 = nodes in LDS, 2 = nodes and costs in LDS. */
int32_t bn_rrt_node_storage(bn_rrt_t *h);
const char *bn_rrt_last_error(void);

/* ------------------------------------------------------------------------------------------------------------------------------
 * The closed-loop RRT planner (csrc/clrrt_kernels.hip): `CLRRT` of src/planners/global_planners/sampling_based/cl_rrt.py for B
 * planners that share the limits and parameters and plan on one risk map (bn_clrrt_set_map) or on one map each
 * (bn_clrrt_set_instance_maps), one wave each: the MT19937 stream of each instance parsed
 * into (x, y, theta) samples, the tree grown by nearest neighbour + Dubins path + pure-pursuit closed-loop simulation on the
 * library's float32 transit and costs, then the goal test, the pick and the concatenated action / state sequences.
 * Errors: the clrrt error string below.
 * ---------------------------------------------------------------------------------------------------------------------------- */
typedef enum bn_clrrt_buffer_id {
    BN_CLRRT_BUF_NODES = 0,            /* (B, max_iterations + 1, 3) float32 */
    BN_CLRRT_BUF_EDGES = 1,            /* (B, max_iterations + 1) int32, the parent; -1 at the root */
    BN_CLRRT_BUF_COSTS = 2,            /* (B, max_iterations + 1) float32 */
    BN_CLRRT_BUF_COUNTS = 3,           /* (B) int32 nodes in the tree */
    BN_CLRRT_BUF_SEQ_LENGTHS = 4,      /* (B, max_iterations + 1) int32 */
    BN_CLRRT_BUF_CONTROLLERS = 5,      /* (B, max_iterations + 1, 4) float32: previous error, integral (linear), the same (angular) */
    BN_CLRRT_BUF_ACTION_SEQS = 6,      /* (B, max_iterations + 1, max_seqs, 2) float32 */
    BN_CLRRT_BUF_STATE_SEQS = 7,       /* (B, max_iterations + 1, max_seqs + 1, 3) float32 */
    BN_CLRRT_BUF_SAMPLES = 8,          /* (B, max_iterations, 3) float32 */
    BN_CLRRT_BUF_SAMPLE_FLAGS = 9,     /* (B, max_iterations) int32: 1 where the sample is the goal node */
    BN_CLRRT_BUF_NEAREST = 10,         /* (B, max_iterations) int32: the nearest node of every iteration */
    BN_CLRRT_BUF_FEASIBLE = 11,        /* (B, max_iterations) int32: 1 where the iteration added a node */
    BN_CLRRT_BUF_PATH_ACTIONS = 12,    /* (B, path_cap, 2) float32, NaN beyond the path */
    BN_CLRRT_BUF_PATH_STATES = 13,     /* (B, path_cap + 1, 3) float32, NaN beyond the path */
    BN_CLRRT_BUF_RESULTS = 14,         /* (B, 6) int32: found, picked node (-1), path length, near-goal nodes, error (BN_ERR_STATE: the path
                                          does not fit path_cap and was not written), node count */
    BN_CLRRT_BUF_STEER_ACTIONS = 15,   /* bn_clrrt_steer_async: (B, max_seqs, 2) float32 */
    BN_CLRRT_BUF_STEER_STATES = 16,    /* (B, max_seqs + 1, 3) float32 */
    BN_CLRRT_BUF_STEER_PATHS = 17,     /* (B, 64, 2) float64: the truncated reference path, NaN beyond it */
    BN_CLRRT_BUF_STEER_TARGETS = 18,   /* (B, max_seqs) int32: the target point's index at every step */
    BN_CLRRT_BUF_STEER_RESULTS = 19,   /* (B, 4) int32: feasible, length, Dubins word (LSL RSR RSL LSR RLR LRL), path points */
    BN_CLRRT_BUF_STEER_COSTS = 20,     /* (B) float32 */
    BN_CLRRT_BUF_STEER_CONTROLLERS = 21, /* (B, 4) float64: the controllers' state after the steer */
    BN_CLRRT_BUF_MT_STATE = 22,        /* (B, 624) uint32: the MT19937 state block of every instance's stream */
    BN_CLRRT_BUF_MT_POS = 23           /* (B) int32: the next word of the block */
} bn_clrrt_buffer_id;

typedef struct bn_clrrt_config {
    uint32_t struct_size;          /* sizeof(bn_clrrt_config), set by the init function */
    int32_t device_id;
    int32_t num_instances;         /* B */
    int32_t max_iterations;        /* cl_rrt.py:34; at most 2047 (the nodes live in LDS) */
    int32_t max_seqs;              /* cl_rrt.py:37: closed-loop steps per steer */
    int32_t path_cap;              /* actions the path buffers hold per instance; 0 = min(max_iterations * max_seqs, 65536) */
    int32_t grid_size;             /* G: the risk map is (G, G) */
    int32_t reserved;
    double resolution;             /* a power of two */
    double x_limits[2], y_limits[2];
    double delta_distance;         /* cl_rrt.py:35, at most 12 */
    double goal_sample_rate;       /* cl_rrt.py:36 */
    double goal_threshold;         /* cl_rrt.py:38 */
    double delta_t;                /* the PID controllers' time step */
    double transit_dt;             /* UnicycleModel.transit's delta_t (its default 0.1: CLRRT does not pass its own) */
    double u_min[2], u_max[2];     /* action bounds of the transit */
    uint64_t seed;                 /* 0 ... 2^32 - 1 */
} bn_clrrt_config;

typedef struct bn_clrrt bn_clrrt_t;
void bn_clrrt_config_init(bn_clrrt_config *cfg);
/* Arguments are checked before the device is touched; without a device BN_ERR_NO_DEVICE ("no CPU fallback"). */
int bn_clrrt_create(const bn_clrrt_config *cfg, bn_clrrt_t **out);
void bn_clrrt_destroy(bn_clrrt_t *h);
/* The risk map the dynamics reads, HOST (G, G) float32 (traversability = 1 - clamp(risk, 0, 1)), shared by the instances; the
 * goal (2) the costs of bn_clrrt_steer_async run against; the stuck threshold.  Synchronous.  Ends bn_clrrt_set_instance_maps. */
int bn_clrrt_set_map(bn_clrrt_t *h, const float *risk, const float *goal, double stuck_threshold);
/* One risk map per instance: risks (B, G, G) float32, `where` a bn_mem_kind; a device source is copied device to device on
 * `stream`, a host source is consumed before the call returns.  From here on instance b's plans and steers read map b, until
 * bn_clrrt_set_map returns the handle to its shared map; the goal of bn_clrrt_steer_async stays bn_clrrt_set_map's (zeros before
 * it).  Waits for the handle's latest launch.  The B maps are allocated by the first call: a handle that never makes it holds
 * the shared map only. */
int bn_clrrt_set_instance_maps(bn_clrrt_t *h, void *stream, const void *risks, int where, double stuck_threshold);
/* One forward() of every instance on `stream`: starts HOST (B, 3) float32 states, goals HOST (B, 3) float32 goal nodes (x, y,
 * heading; the costs run against (x, y)), consumed before the call returns; a position out of the limits is BN_ERR_INVALID and
 * nothing is launched.  seeds as bn_rrt_plan_async. */
int bn_clrrt_plan_async(bn_clrrt_t *h, void *stream, const float *starts, const float *goals, const uint64_t *seeds);
/* The growth, the goal test and the path on the caller's samples (B, max_iterations, 3) float32, `where` a bn_mem_kind. */
int bn_clrrt_grow_from_samples_async(bn_clrrt_t *h, void *stream, const float *starts, const float *goals, const void *samples, int where);
/* One steer per instance with no tree: from_states HOST (B, 3), controller_states HOST (B, 4), targets HOST (B, 3) float32; the
 * results are the BN_CLRRT_BUF_STEER_* buffers. */
int bn_clrrt_steer_async(bn_clrrt_t *h, void *stream, const float *from_states, const float *controller_states, const float *targets);
int bn_clrrt_sync(bn_clrrt_t *h);
/* Device pointer and size in bytes of one of the handle's buffers (bn_clrrt_buffer_id); valid until the handle is destroyed. */
int bn_clrrt_device_buffer(bn_clrrt_t *h, int which, void **ptr, size_t *bytes);
int32_t bn_clrrt_path_cap(bn_clrrt_t *h);
const char *bn_clrrt_last_error(void);

/*
 * The CL-RRT plan-follow-replan loop (csrc/clrrt_loop.hip): the reference's driver loop test/test_cl_rrt.py:167-200
 * for the B environments of h (bn_mppi_env_attach) and the B instances of a CL-RRT handle c on the same grid.  Per rover, with t
 * counting LOOP ITERATIONS: a plan where one is needed (t = 0, or flagged by the previous iteration); for t > 0 the deviation
 * min over all L + 1 planned states of |plan_xy - state_xy| in float32, and deviation > 1 flags a replan -- that iteration takes
 * no step; else action_seq[action_index++] through PlanetaryEnv.step with the slip draw of iteration t (z row t of the call, or
 * Philox keyed by (env seed, t)); terminated stops the rover (GOAL), then elapsed > time_limit (TIME_LIMIT).  Where the reference
 * raises or fails the rover alone stops with a status.  The follow kernel runs every rover to the call's end or to its next
 * replan; the host reads one counter per ROUND of replans and runs c's kernels for the flagged rovers only.  c's streams are
 * seeded by the reset and continue across a rover's replans; c serves the loop alone between a reset and the episode's end, and run / set_plans
 * take the handle the reset was given (another one is BN_ERR_INVALID).
 */
typedef enum bn_clrrt_loop_status {
    BN_CL_RUNNING = 0,
    BN_CL_GOAL = 1,             /* is_terminated: the loop breaks (test_cl_rrt.py:194-196)                                  */
    BN_CL_TIME_LIMIT = 2,       /* is_truncated (:198-200)                                                                  */
    BN_CL_NO_PLAN = 3,          /* forward returned (None, None): the reference's loop fails on it with a TypeError         */
    BN_CL_NO_SEQUENCE = 4,      /* the root is the cheapest node within the goal threshold: forward raises                  */
    BN_CL_PLAN_EXHAUSTED = 5,   /* action_index == L: the reference's IndexError                                            */
    BN_CL_PATH_OVERFLOW = 6,    /* the plan does not fit c's path_cap                                                        */
    BN_CL_OUT_OF_BOUNDS = 7     /* forward's ValueError("Start or goal position is out of bounds.")                         */
} bn_clrrt_loop_status;
typedef enum bn_clrrt_loop_event {
    BN_CL_EVENT_STEP = 0,       /* the iteration took an environment step */
    BN_CL_EVENT_REPLAN = 1,     /* deviation > 1: a replan is flagged, no step */
    BN_CL_EVENT_FROZEN = 2      /* the rover has stopped (from the iteration on at which a status without a step was set) */
} bn_clrrt_loop_event;
/* A new episode (test_cl_rrt.py:167): iteration 0, no plan, statuses cleared; goal_nodes HOST (B, 3) (x, y, heading: the
 * heading of the rover's FIRST forward, kept for every replan) and seeds HOST (B) uint64 of c's MT19937 streams.  Verifies that
 * c's B, grid size, resolution, limits and action bounds are h's.  delta_t and time_limit: PlanetaryEnv's, in double as the
 * reference holds them: it accumulates elapsed += delta_t in float64 and stops a rover once elapsed > time_limit; delta_t must
 * round to the float32 step of bn_mppi_env_attach. */
int bn_clrrt_loop_reset(bn_mppi_t *h, bn_clrrt_t *c, const float *goal_nodes, const uint64_t *seeds, double delta_t, double time_limit);
/* n loop iterations on h's stream from states_device (B, 3), which receives the final states.  z_device (n, B) slip draws or
 * NULL; samples_device (P, B, max_iterations, 3) or NULL: rover b's p-th plan since the reset grows from table p instead of
 * its stream, and a rover that needs a plan beyond P stops with BN_CL_NO_PLAN (teacher forcing).  flags bit 0: read the plan
 * from global memory even where it fits the LDS budget (test knob; the outputs are bit-identical).  Synchronises once per
 * round of replans.  follow_ms (may be NULL): the time between HIP events around the follow launches, summed. */
int bn_clrrt_loop_run(bn_mppi_t *h, bn_clrrt_t *c, int32_t n, float *states_device, const float *z_device,
                      const float *samples_device, int32_t num_tables, uint32_t flags, float *follow_ms);
/* The latest run's log (any pointer may be NULL), rows by iteration of the call: states (n+1,B,3) with [0] the call's start,
 * rewards (n,B), actions (n,B,2), deviations (n,B), plan_index (n,B) int32, events (n,B) int32 bn_clrrt_loop_event; a row
 * without a step holds the state and NaN elsewhere (a flagged replan keeps its deviation).  Per rover (B) int32: done_iter
 * (the iteration its status was set at, or -1), status, plans (forward calls), steps (environment steps) since the reset. */
int bn_clrrt_loop_log(bn_mppi_t *h, float *states, float *rewards, float *actions, float *deviations, int32_t *plan_index,
                      int32_t *events, int32_t *done_iter, int32_t *status, int32_t *plans, int32_t *steps);
/* The latest run's log where it lies, for readers on the device (bn_episode_score): states (row_capacity + 1, B, 3) and rewards
 * (row_capacity, B), laid out by the rows the log holds, of which the first n_iterations (+ 1) are the run's; done_step (B) int32:
 * done_iter where the status is BN_CL_GOAL, else -1; stopped (B) int32: the status where it is neither RUNNING, GOAL nor
 * TIME_LIMIT, else 0.  The two words are written on h's stream behind the run (done_iter counts from the reset: they index the
 * log of a run that started there).  Any pointer may be NULL; nothing is copied or synchronised. */
int bn_clrrt_loop_episode_buffers(bn_mppi_t *h, const float **states_device, const float **rewards_device,
                                  const int32_t **done_step_device, const int32_t **stopped_device, int32_t *n_iterations, int32_t *row_capacity);
/* ... and the rovers' status (bn_clrrt_loop_status) and plans (forward calls since the reset), (B) int32 each, as that run left them. */
int bn_clrrt_loop_rover_buffers(bn_mppi_t *h, const int32_t **status_device, const int32_t **plans_device);
/* Teacher forcing: actions HOST (B, Lmax, 2), states HOST (B, Lmax + 1, 3) and lengths HOST (B) int32 (1 <= L <= min(Lmax,
 * path_cap)) become the rovers' current plans, action_index 0, no replan pending; iteration >= 0 also sets every rover's
 * iteration counter.  The follow kernel can be driven with this alone. */
int bn_clrrt_loop_set_plans(bn_mppi_t *h, bn_clrrt_t *c, const float *actions, const float *states, const int32_t *lengths,
                            int32_t max_length, int32_t iteration);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Exact-GP slip prediction (csrc/gp_kernels.hip): the per-class GP regressors behind
 * TraversabilityPredictor.predict (classifier_and_regressor.py:42-72; slip_regressors/gpr.py: ExactGP, ConstantMean,
 * ScaleKernel(RBFKernel) with one lengthscale, GaussianLikelihood, 1-D input).  With training inputs x[n], targets y[n],
 * constant mean c, outputscale s, lengthscale l and noise:
 *     k(a, b) = s exp(-(a - b)^2 / (2 l^2))          K = k(x, x) + noise I = L L^T (Cholesky, L lower)
 *     alpha = K^-1 (y - c)                            linv = L^-1 (lower triangular)
 * and for a cell of slope phi
 *     mean = c + k(phi, x) . alpha                    v = linv k(x, phi)
 *     var  = max(s - |v|^2, 0) + noise                std = sqrt(var)            (the likelihood's noise is part of var)
 * A caller produces alpha and linv with LAPACK (dpotrf, dpotrs, dtrtri) in float64 for bn_gp_create, or lets the library
 * factorise on the device (bn_gp_fit_create, bn_gp_fit_set_hyperparameters, bn_gp_fit_finish below); no jitter is added either
 * way.  The device evaluates every line above in float64 and rounds only the outputs.
 * Errors: the gp error string below.
 * ---------------------------------------------------------------------------------------------------------------------------- */
typedef struct bn_gp bn_gp_t;
/* The largest n bn_gp_create takes: 10240 (640 row blocks of 16; L^-1 is 420 MB on the device at that size).  Regressors of up to
 * 1024 points keep the k(x, phi) tile of 16 cells in LDS; larger ones run on a second kernel that walks L^-1 in slabs of 512 rows
 * and regenerates k(x, phi) per slab, 64 cells per workgroup.  bn_gp_predict_async picks per class; both may serve one call. */
int32_t bn_gp_max_points(void);
/* One regressor on device_id from HOST arrays: x (n), alpha (n), linv (n, n) row-major of which the lower triangle is read.
 * Checked before the device is touched: 1 <= n <= bn_gp_max_points(), every value finite, outputscale, lengthscale and
 * noise > 0 (BN_ERR_INVALID); without a device BN_ERR_NO_DEVICE ("no CPU fallback").  Synchronous. */
int bn_gp_create(int32_t device_id, int32_t n, const double *x, const double *alpha, const double *linv, double constant,
                 double outputscale, double lengthscale, double noise, bn_gp_t **out);
void bn_gp_destroy(bn_gp_t *h);
/* Bytes of device workspace bn_gp_predict_async needs: 4 num_maps cells + 4 num_maps (3 num_classes + 1), each part rounded
 * up to 256.  It does not grow with n.  0 for arguments out of range. */
size_t bn_gp_workspace_bytes(int32_t num_maps, int64_t cells, int32_t num_classes);
/* mean and std of num_maps maps of `cells` cells each on `stream`, two launches, no synchronisation: regressors is a HOST table
 * of num_classes (<= 32) handles of device_id, NULL where a class has none; slopes (num_maps, cells) float32 and classes
 * (num_maps, cells) int32 on the device; mean and std (num_maps, cells) on the device, float32 or (f64_outputs = 1) float64.  A
 * cell whose class is outside [0, num_classes) or has no regressor gets mean 0 and std 0.  The workspace and the regressors
 * must stay alive until the stream has run the launches. */
int bn_gp_predict_async(int32_t device_id, void *stream, bn_gp_t *const *regressors, int32_t num_classes, int32_t num_maps,
                        int64_t cells, const float *slopes_device, const int32_t *classes_device, void *mean_device,
                        void *std_device, int32_t f64_outputs, void *workspace_device, size_t workspace_bytes);
const char *bn_gp_last_error(void);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Fitting the GP slip regressors on the device (csrc/gp_fit_kernels.hip): RegressorTrainer.train's Adam on the
 * exact marginal log-likelihood (trainers/regressor_trainer.py:128-170), in float64, and the factorisation behind a bn_gp_t
 * without host LAPACK.  Raw parameters theta = (constant, raw_outputscale, raw_lengthscale, raw_noise), all 0 at creation as in
 * gpytorch; c = constant, s = softplus(raw_outputscale), l = softplus(raw_lengthscale), noise = softplus(raw_noise) +
 * noise_lower_bound;
 *     K = s exp(-(x - x')^2 / (2 l^2)) + noise I = L L^T      r = y - c      alpha = K^-1 r
 *     loss = [ r . alpha + 2 sum log L_ii + n log 2 pi ] / (2 n)               (the negative marginal log-likelihood over n)
 *     dloss/dc = -sum alpha / n        dloss/dpsi = tr((K^-1 - alpha alpha^T) dK/dpsi) / (2 n),  psi in {s, l, noise}
 * and the gradient with respect to the raw parameters by dpsi/draw = sigmoid(raw).  No jitter is added anywhere: a pivot that is
 * not positive and finite sets the handle's status to 1 with the iteration number, and every launch enqueued behind it returns
 * at once.  Every sum runs in an order fixed by n alone (no floating-point atomics): equal inputs give equal bits.
 * Errors: the gp fit error string below.
 * ---------------------------------------------------------------------------------------------------------------------------- */
typedef struct bn_gp_fit bn_gp_fit_t;
/* Bytes of device memory a fit handle of n points holds: with np = n rounded up to 32 and T = np / 32,
 *     2 np^2 8 (K then L, and L^-1) + 8192 T (the inverses of L's diagonal tiles) + 32 np (x, y, z, alpha)
 *     + 12 T (T + 1) (three gradient partials per tile of K^-1) + 131072 (the loss history) + the state block,
 * 1.68 GB at n = 10240.  0 for n outside [1, bn_gp_max_points()]. */
size_t bn_gp_fit_workspace_bytes(int32_t n);
/* A fit handle on device_id from HOST arrays x (n) and y (n).  Checked before the device is touched: 1 <= n <= bn_gp_max_points(),
 * x and y finite, noise_lower_bound finite and >= 0 (gpytorch's default is 1e-4) (BN_ERR_INVALID); without a device
 * BN_ERR_NO_DEVICE ("no CPU fallback").  theta = 0.  Synchronous. */
int bn_gp_fit_create(int32_t device_id, int32_t n, const double *x, const double *y, double noise_lower_bound, bn_gp_fit_t **out);
void bn_gp_fit_destroy(bn_gp_fit_t *h);
/* theta = raw[4]; clears Adam's moments, the history, the status and the iteration count.  Synchronises. */
int bn_gp_fit_set_raw(bn_gp_fit_t *h, const double *raw);
/* The ACTUAL hyperparameters directly (all finite, the last three > 0), for bn_gp_fit_finish alone: the raw parameters and the
 * gradient are NaN afterwards.  Clears what bn_gp_fit_set_raw clears.  Synchronises. */
int bn_gp_fit_set_hyperparameters(bn_gp_fit_t *h, double constant, double outputscale, double lengthscale, double noise);
/* Loss and gradient at the current theta on `stream`, no update, no synchronisation. */
int bn_gp_fit_evaluate_async(bn_gp_fit_t *h, void *stream);
/* `iterations` (>= 0) steps of torch.optim.Adam's update (lr > 0, betas in [0, 1), eps >= 0; bias-corrected, no weight decay) on
 * `stream` without a host round trip: per step one evaluation, the loss appended to the history, theta and the moments updated.
 * A handle records up to 16384 iterations. */
int bn_gp_fit_run_async(bn_gp_fit_t *h, void *stream, int32_t iterations, double lr, double beta1, double beta2, double eps);
/* Synchronises the last stream used and reads theta, the gradient and loss of the last evaluation, the status (0, or 1: a
 * factorisation failed) and the iteration it failed in (-1 if none).  Any output pointer may be NULL. */
int bn_gp_fit_read(bn_gp_fit_t *h, double *raw, double *grad, double *loss, int32_t *status, int32_t *failed_iteration);
/* Synchronises; hyp[4] = (constant, outputscale, lengthscale, noise) as the next evaluation will use them. */
int bn_gp_fit_hyperparameters(bn_gp_fit_t *h, double *hyp);
/* Synchronises; copies min(completed iterations, capacity) losses, oldest first, and returns the number of completed iterations
 * (or a negative error code). */
int32_t bn_gp_fit_history(bn_gp_fit_t *h, double *losses, int32_t capacity);
/* Factorises at the current hyperparameters on `stream` and hands back an ordinary regressor for bn_gp_predict_async: alpha and
 * L^-1 are written on the device in the handle's own order, nothing of size n^2 crosses the bus.  Synchronises.  BN_ERR_STATE
 * when the matrix is not numerically positive definite ("no jitter is added").  The regressor outlives the fit handle. */
int bn_gp_fit_finish(bn_gp_fit_t *h, void *stream, bn_gp_t **out);
const char *bn_gp_fit_last_error(void);

/* ------------------------------------------------------------------------------------------------------------------------------
 * The U-Net terrain classifier (csrc/unet_kernels.hip, csrc/unet_host.cpp): the first half of
 * TraversabilityPredictor.predict, colours (num_maps, 3, H, W) in [0, 1] -> logits, softmax probabilities and class maps.  The
 * network is terrain_classifiers/unet.py's Unet(encoder "resnet18", classes): a ResNet-18 encoder, five decoder blocks (2x
 * nearest upsample, concatenation with the skip feature, two 3x3 convolutions) and a 3x3 head, in eval mode: every BatchNorm is
 * folded into its convolution BEFORE upload, so the library sees 31 convolutions with a bias each.  Float32 throughout, on the
 * exact float32 MFMA; an output's bits depend on the parameters and on that map's pixels only.
 *
 * The packed parameters, float32: per convolution its weights (cout, cin, k, k) row-major, then its bias (cout), in this order:
 *     encoder.conv1 (64, 3, 7, 7);
 *     encoder.layer1 ... layer4 with widths 64, 128, 256, 512, per layer: block 0 conv1, block 0 conv2, [layers 2-4: block 0
 *         downsample (1x1)], block 1 conv1, block 1 conv2;
 *     decoder.blocks.0 ... 4: conv1 (cout, cin + cskip, 3, 3), conv2 (cout, cout, 3, 3), with cin = 512, 256, 128, 64, 32, cskip =
 *         256, 128, 64, 64, 0 and cout = 256, 128, 64, 32, 16; the input channels are [upsampled, skip] in that order;
 *     segmentation_head.0 (classes, 16, 3, 3).
 * Range: H and W multiples of 32 in [32, 2048], num_maps in [1, 4096], num_maps H W <= 2^24.
 * Errors: the unet error string below.
 * ---------------------------------------------------------------------------------------------------------------------------- */
typedef struct bn_unet bn_unet_t;
/* Floats of packed parameters for `classes` terrain classes (14 323 722 at 10); 0 for classes outside [1, 32]. */
int64_t bn_unet_param_count(int32_t classes);
/* A classifier on device_id from the HOST array of packed parameters.  Checked before the device is touched: 1 <= classes <= 32,
 * count == bn_unet_param_count(classes), every value finite (BN_ERR_INVALID); without a device BN_ERR_NO_DEVICE ("no CPU
 * fallback").  Re-lays every convolution out as the kernel reads it ([k][cout], padded with zeros).  Synchronous. */
int bn_unet_create(int32_t device_id, int32_t classes, const float *params_host, int64_t count, bn_unet_t **out);
void bn_unet_destroy(bn_unet_t *h);
/* Bytes of device workspace one forward of num_maps maps of H x W needs: every activation of the network, each rounded up to
 * 256 bytes, and room for the logits of 32 classes (used when the caller passes none).  0 for arguments out of range or H, W not
 * multiples of 32. */
size_t bn_unet_workspace_bytes(int32_t num_maps, int32_t H, int32_t W);
/* One forward on `stream`: 32 launches (33 with probabilities or classes), no synchronisation, no allocation.  colors_device
 * (num_maps, 3, H, W) float32; any of logits_device (num_maps, classes, H, W) float32, probabilities_device (same shape, softmax
 * over the classes) and classes_device (num_maps, H, W) int32 (argmax of the logits, the lowest index wins a tie) may be NULL.  The
 * handle and the workspace must stay alive until the stream has run the launches. */
int bn_unet_forward_async(bn_unet_t *h, void *stream, int32_t num_maps, int32_t H, int32_t W, const float *colors_device,
                          float *logits_device, float *probabilities_device, int32_t *classes_device, void *workspace_device,
                          size_t workspace_bytes);
/* Where a forward of this shape leaves feature `index` in its workspace: 0 the stem (after bn1 + ReLU), 1-4 layer1 ... layer4,
 * 5-9 decoder blocks 0 ... 4; each (num_maps, channels, height, width) float32 at offset_bytes. */
int bn_unet_feature_layout(int32_t num_maps, int32_t H, int32_t W, int32_t index, size_t *offset_bytes, int32_t *channels,
                           int32_t *height, int32_t *width);
/* Bytes of workspace bn_unet_conv2d_async needs for the re-laid weights; 0 unless 1 <= cin, cout <= 4096 and ksize is 1, 3 or 7. */
size_t bn_unet_conv2d_workspace_bytes(int32_t cin, int32_t cout, int32_t ksize);
/* The network's one fused convolution on caller tensors, all on the device (two launches: the weight re-layout, the convolution):
 *     out = [relu]( conv2d([up2x](a) ++ skip, weights, stride, pad) + bias [+ residual] )
 * a (num_maps, ca, hin, win), or (num_maps, ca, hin / 2, win / 2) with upsample = 1 (2x nearest); skip (num_maps, cb, hin, win) or
 * NULL with cb = 0; weights (cout, ca + cb, ksize, ksize); bias (cout) or NULL; residual of out's shape or NULL; ksize 1, 3 or 7,
 * stride 1 or 2, pad 0 ... 3, zero padding; out (num_maps, cout, (hin + 2 pad - ksize) / stride + 1, likewise for win). */
int bn_unet_conv2d_async(int32_t device_id, void *stream, const float *a_device, int32_t ca, const float *skip_device, int32_t cb,
                         int32_t upsample, int32_t num_maps, int32_t hin, int32_t win, const float *weights_device,
                         const float *bias_device, int32_t cout, int32_t ksize, int32_t stride, int32_t pad,
                         const float *residual_device, int32_t relu, float *out_device, void *workspace_device, size_t workspace_bytes);
/* The network's max-pool (3x3, stride 2, pad 1, padding counts as -inf) on `planes` device images of hin x win:
 * out (planes, (hin - 1) / 2 + 1, (win - 1) / 2 + 1). */
int bn_unet_maxpool_async(int32_t device_id, void *stream, const float *in_device, int64_t planes, int32_t hin, int32_t win,
                          float *out_device);
const char *bn_unet_last_error(void);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Training the U-Net terrain classifier (csrc/segtrain_kernels.hip, csrc/segtrain_host.cpp): the reference's
 * trainers/classifier_trainer.py on the device -- the network above in TRAINING mode (BatchNorm on batch statistics), the mean
 * cross-entropy over all cells, the backward pass and Adam.  Float32 tensors; convolutions (forward, backward-data,
 * backward-weight) on the exact float32 MFMA; every reduction and every elementwise formula of BatchNorm, the loss and Adam in
 * float64 from the float32 operands, rounded once.  No atomics: two runs from the same state give the same bits.
 *
 * The packed UNFOLDED parameters, float32, in the order of the convolutions above: per convolution its weights (cout, cin, k, k),
 * then its BatchNorm's gamma, beta, running mean and running variance (cout each); the head has its bias (classes) instead of
 * those four.  Gradients, m and v are read in the same layout with zeros in the place of the running statistics.
 * Range: that of bn_unet_workspace_bytes, and num_maps (H / 32) (W / 32) > 1 (more than one value per channel at the bottleneck).
 * Errors: the segtrain error string below.
 * ---------------------------------------------------------------------------------------------------------------------------- */
typedef struct bn_segtrain bn_segtrain_t;
/* Floats of packed unfolded parameters for `classes` classes; 0 for classes outside [1, 32]. */
int64_t bn_segtrain_param_count(int32_t classes);
/* A trainer on device_id from the HOST array of packed parameters: it holds the parameters, their gradients, Adam's m and v (zero)
 * and the step count (zero).  Checked before the device is touched like bn_unet_create; BN_ERR_NO_DEVICE ("no CPU fallback"). */
int bn_segtrain_create(int32_t device_id, int32_t classes, const float *params_host, int64_t count, bn_segtrain_t **out);
void bn_segtrain_destroy(bn_segtrain_t *h);
/* Bytes of device workspace one step on num_maps maps of H x W needs (every activation is kept for the backward pass); 0 out of
 * range. */
size_t bn_segtrain_workspace_bytes(int32_t num_maps, int32_t H, int32_t W);
/* Training-mode forward, loss and backward on `stream`, no synchronisation: colors_device (num_maps, 3, H, W) float32,
 * targets_device (num_maps, H, W) int64 in [0, classes) (the caller checks the range; a value outside contributes nothing),
 * loss_device one float.  The gradients stay in the handle; no parameter, running statistic or step count changes. */
int bn_segtrain_grad_async(bn_segtrain_t *h, void *stream, int32_t num_maps, int32_t H, int32_t W, const float *colors_device,
                           const int64_t *targets_device, float *loss_device, void *workspace_device, size_t workspace_bytes);
/* The same, then the running statistics (momentum 0.1, unbiased variance) and one step of torch.optim.Adam on every trainable
 * parameter; the step count goes up by one.  Fully enqueued on `stream`; loss_device may point into an array of slots. */
int bn_segtrain_step_async(bn_segtrain_t *h, void *stream, int32_t num_maps, int32_t H, int32_t W, const float *colors_device,
                           const int64_t *targets_device, double lr, double beta1, double beta2, double eps, double weight_decay,
                           float *loss_device, void *workspace_device, size_t workspace_bytes);
/* Copies to the host, after a device synchronise: what = 0 the parameters, 1 the gradients, 2 Adam's m, 3 Adam's v; count ==
 * bn_segtrain_param_count(classes). */
int bn_segtrain_read(bn_segtrain_t *h, int32_t what, float *host, int64_t count);
/* Steps taken so far (BatchNorm's num_batches_tracked grows by the same number); -1 for a null handle. */
int64_t bn_segtrain_steps(bn_segtrain_t *h);
/* Single layers on caller tensors, all on the device, for the layer-level tests.
 * conv2d_backward: the gradients of bn_unet_conv2d_async's convolution (no bias, residual or ReLU) given grad_out (num_maps, cout,
 * hout, wout): grad_weight (cout, ca + cb, ksize, ksize), grad_a of a's shape (the 2 x 2 sum with upsample = 1), grad_skip of the
 * skip's shape; any of the three may be NULL.  accumulate = 1 adds grad_a and grad_skip to what the destinations hold.  pad <=
 * ksize - 1.  The workspace size takes cin = ca + cb; 0 for arguments out of range. */
size_t bn_segtrain_conv2d_backward_workspace_bytes(int32_t num_maps, int32_t cin, int32_t hin, int32_t win, int32_t cout, int32_t ksize,
                                                   int32_t stride, int32_t pad);
int bn_segtrain_conv2d_backward_async(int32_t device_id, void *stream, const float *a_device, int32_t ca, const float *skip_device, int32_t cb,
                                      int32_t upsample, int32_t num_maps, int32_t hin, int32_t win, const float *weights_device, int32_t cout,
                                      int32_t ksize, int32_t stride, int32_t pad, const float *grad_out_device, float *grad_weight_device,
                                      float *grad_a_device, float *grad_skip_device, int32_t accumulate, void *workspace_device,
                                      size_t workspace_bytes);
/* y = [relu]((x - mean) gamma / sqrt(var + 1e-5) + beta [+ residual]) on the batch statistics of x (num_maps, channels, cells);
 * stats_device receives 2 channels doubles (mean, 1 / sqrt(var + eps)); the running statistics, if given, are updated in place. */
int bn_segtrain_batchnorm_forward_async(int32_t device_id, void *stream, const float *x_device, int32_t num_maps, int32_t channels, int64_t cells,
                                        const float *gamma_device, const float *beta_device, const float *residual_device, int32_t relu,
                                        float *running_mean_device, float *running_var_device, float *y_device, double *stats_device);
/* Its backward from the saved x, y and stats: grad_x (may be grad_out's buffer), grad_residual (the gradient behind the ReLU mask,
 * or NULL), grad_gamma, grad_beta; sums_device is scratch of 2 channels doubles. */
int bn_segtrain_batchnorm_backward_async(int32_t device_id, void *stream, const float *grad_out_device, const float *y_device,
                                         const float *x_device, const double *stats_device, const float *gamma_device, int32_t relu,
                                         int32_t num_maps, int32_t channels, int64_t cells, float *grad_x_device, float *grad_residual_device,
                                         float *grad_gamma_device, float *grad_beta_device, double *sums_device);
/* The backward of bn_unet_maxpool_async: a cell receives a window's gradient iff it is the window's first maximum in row-major
 * order. */
int bn_segtrain_maxpool_backward_async(int32_t device_id, void *stream, const float *x_device, const float *grad_out_device, int64_t planes,
                                       int32_t hin, int32_t win, float *grad_x_device, int32_t accumulate);
/* loss = -mean log softmax(logits)[target] over num_maps x cells cells and, unless NULL, grad_logits = (softmax - onehot) / (num_maps
 * cells); the workspace holds 8 bytes per cell. */
int bn_segtrain_cross_entropy_async(int32_t device_id, void *stream, const float *logits_device, const int64_t *targets_device, int32_t num_maps,
                                    int32_t classes, int64_t cells, float *loss_device, float *grad_logits_device, void *workspace_device,
                                    size_t workspace_bytes);
/* Step number `step` (from 1) of torch.optim.Adam on n parameters in place. */
int bn_segtrain_adam_async(int32_t device_id, void *stream, float *params_device, const float *grads_device, float *m_device, float *v_device,
                           int64_t n, int64_t step, double lr, double beta1, double beta2, double eps, double weight_decay);
const char *bn_segtrain_last_error(void);

/* ---- The dataset stage: slip observations and the regressor trainer's per-class gather -------------------------
 * No handle: device pointers, the caller's stream, the caller's workspace; nothing synchronises.  Errors: bn_dataset_last_error().
 *
 * The observation stream: map m (its global index in the split, below 2^32) has Philox blocks j = 0 ..
 * ceil(cells / 4) - 1; block j is Philox4x32-10 of the counter {j, m, epoch, 'OBSV' = 0x4F425356} under the key (lo(seed), hi(seed));
 * Box-Muller of the words (x, y) gives z of cells 4j and 4j + 1, of (z, w) cells 4j + 2 and 4j + 3; a ragged last block drops the
 * rest.  slip = z * std + mean as a rounded product and a rounded sum (Normal.sample).
 *
 * sample_slips: mean, std and slips are (num_maps, cells) float32; row r is map first_map + r, so a split drawn in chunks equals
 * the split drawn at once.  z_device (num_maps, cells), unless NULL, replaces the stream (parity tests). */
int bn_dataset_sample_slips_async(int32_t device_id, void *stream, const float *mean_device, const float *std_device, const float *z_device,
                                  int64_t num_maps, int64_t cells, int64_t first_map, uint64_t seed, uint32_t epoch, float *slips_device);
/* Bytes of device workspace one gather over num_maps maps and num_classes classes needs; 0 for arguments out of range. */
size_t bn_dataset_gather_workspace_bytes(int64_t num_maps, int32_t num_classes);
/* RegressorTrainer.load_data (regressor_trainer.py:90-126).  slopes, slips, mean, std: (num_maps, cells) float32; classes:
 * (num_maps, cells) int32; order_device: (num_maps) int64, the maps in visiting order (NULL: 0, 1, ...; an entry outside
 * [0, num_maps) names no map).  Row k of x and y, (num_classes, cap) float32, receives slopes[m][classes[m] == k] and
 * slips[m][classes[m] == k] for m in visiting order, row-major inside a map, cut at cap; what lies beyond counts[k] is not written.
 * counts (num_classes) int32 = min(totals, cap); totals (num_classes) int64.  A class value outside [0, num_classes) selects nothing
 * (the reference's -1 "unassigned").  slips_device == NULL: the kept cells' observations are drawn in the kernel from mean and std
 * with (seed, epoch) and the map's index as m -- bit for bit the gather over bn_dataset_sample_slips_async's output (first_map 0).
 * Three launches (count, scan, scatter), integer ranks, no atomics on the outputs: the result does not depend on the launch
 * geometry and two runs give the same bits.  num_classes <= 64, cap >= 1, num_maps < 2^32, cells < 2^31. */
int bn_dataset_gather_async(int32_t device_id, void *stream, const float *slopes_device, const float *slips_device, const float *mean_device,
                            const float *std_device, const int32_t *classes_device, const int64_t *order_device, int64_t num_maps, int64_t cells,
                            int32_t num_classes, int32_t cap, uint64_t seed, uint32_t epoch, float *x_device, float *y_device,
                            int32_t *counts_device, int64_t *totals_device, void *workspace_device, size_t workspace_bytes);
const char *bn_dataset_last_error(void);

/* Test hook: the library's device arithmetic (DESIGN.md "Arithmetic spec") applied elementwise to n device floats:
 * fn 0 = correctly rounded sqrt, 1 / 2 = sin / cos of the spec, 3 = heading wrap (theta + pi) % 2pi - pi with
 * torch.remainder semantics (robot_model.py:90), 4 = its in-loop form, 5 = the sqrt for zero / normal finite arguments.  Lets the tests compare the kernels' building
 * blocks with the oracle's one value at a time.
 * fn 6 = the atan2f of DWA's sub-goal bearing (dwa.py:272), on PAIRS: in_device holds 2 n floats, record i = (dy, dx) =
 * (in[2 i], in[2 i + 1]), and out_device n floats, out[i] = atan2f(dy, dx) as the sub-goal kernels evaluate it. */
int bn_device_math_eval(int32_t fn, const float *in_device, float *out_device, int64_t n, void *stream);
/* Test hook: the generator every noise stream is built from, on n caller-supplied device records (uint32 words):
 * fn 0 = Philox4x32-10, 1 = Philox4x32 with the per-rollout streams' eight rounds: record 6 words (c0, c1, c2, c3, k0, k1)
 * -> 4 words; fn 2 = Box-Muller: record 2 words (a, b) -> 2 floats (z0, z1) as bits.  The kernels' own inline functions. */
int bn_device_rng_eval(int32_t fn, const uint32_t *in_device, uint32_t *out_device, int64_t n, void *stream);

const char *bn_last_error(void);
int bn_mppi_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* BENCHNAV_MPPI_H */
