// mppi_handle.h -- the planner handle behind bn_mppi_t and what the host files of the C ABI share (mppi_capi.cpp, mppi_plan.cpp,
// mppi_solve.cpp, mppi_paced.cpp, mppi_shard.cpp, mppi_env.cpp, mppi_loops.cpp, mppi_query.cpp): the constants of the launch policy, the handle with
// its buffer tables (bn_host.h), the functions more than one file calls, the HIP check and the tables' fail adapter, the device
// binding of an entry point, and the request words of the host-paced loop.  Private, host only, not installed.
#pragma once
#include "../../include/benchnav_mppi.h"
#include "mppi_kernels.h"
#include "bn_host.h"
#include "episode_log.h"

#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

namespace bn { struct ClrrtRover; }         // clrrt_view.h (mppi_loops.cpp)

namespace {

constexpr int kProfGroup = 10;
// Experiment switches (environment variables read by the measurement tools under tools/): compiled in only with -DBN_EXPERIMENTS
// (tools/build_variant*.py pass it); the shipped library has none in its entry points.
#ifdef BN_EXPERIMENTS
inline const char *exp_env(const char *name) { return std::getenv(name); }
#else
inline const char *exp_env(const char *) { return nullptr; }
#endif

// Up to this many workgroups per instance every rollout workgroup re-merges the previous solve's partials itself (pipelined mode:
// no merge launch, no ticket round trips); above, the last workgroup of a launch merges (ticket mode).  64 = what the few-rows
// merge takes in one wave; measured at K=4096: 17.1 us per solve pipelined against 21.2 with the ticket merge (tools/k_sweep.py).
constexpr int kPipelinedMaxBlocks = 64;
constexpr int kEagerTailMinBatch = 16;    // overlapped batches of at least this many solves end with their own tail kernel
constexpr int kMaxStreams = 3;            // launches of one overlapped batch in flight at most
constexpr int kSlots = kMaxStreams + 1;   // per-solve buffer slots (see bn_mppi::d_cost)
constexpr size_t kJournalCap = 4096;
constexpr size_t kLaunchLogCap = 256;     // bn_mppi_debug_launch_log keeps the latest this many launches

}  // namespace

struct bn_mppi {
    bn_mppi_config cfg{};
    bn::SolveParams p{};
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int n_maps = 1;
    uint64_t solves = 0;
    bool map_set = false, goal_set = false;
    uint64_t map_epoch = 0, map_epoch_at_solve = 0;   // set_map calls so far / at the latest solve: a re-roll needs the map that solve saw
    // Pipelined mode (K <= 2048): one launch per solve.  The launch of solve i merges solve i-1's
    // per-block statistics in every rollout workgroup (warm start) and carries an aux workgroup that
    // writes solve i-1's tail (U*, X*, weights).  `tail_pending` = the latest solve's tail has not been
    // written yet; flush() launches the finish kernel for it.
    bool pipelined = false;
    bool slow_path = false;          // rollout_wave_kernel + stand-alone tail, two launches per solve: horizons beyond the role kernels' LDS, or the reference-order
                                     // arithmetic together with sampled slip (the reference order by itself runs on every kernel family, one launch per solve)
    bool tail_pending = false;
    // device buffers
    float *d_map = nullptr, *d_state = nullptr, *d_goal = nullptr, *d_mean = nullptr, *d_eps = nullptr;
    float *d_X = nullptr, *d_U = nullptr, *d_w = nullptr, *d_cost_out = nullptr;
    // per-solve buffers rotate over kSlots slots (solve i uses slot i % kSlots): with S launches in flight (see bn_mppi_solve_n_async)
    // solve i+S may start while solve i+1 -- its merge, its aux workgroup -- still reads solve i's slot: S + 1 slots are enough
    float *d_cost[kSlots] = {}, *d_part[kSlots] = {}, *d_state_copy[kSlots] = {};
    float *d_ustar = nullptr, *d_xstar = nullptr, *d_stats = nullptr, *d_scratch = nullptr;
    float *d_mean_used = nullptr;    // the mean the latest finished solve sampled around (re-rolls)
    int *d_idx = nullptr;
    const float *last_eps = nullptr; // noise of the latest solve (caller-owned unless BN_NOISE_HOST_KT2) and its layout
    bn::EpsMode last_mode = bn::kEpsPhilox;
    float *d_slip_std = nullptr;     // sampled-slip mode
    float *d_ustar2[kSlots] = {}, *d_stats2[kSlots] = {};   // ticket-merge outputs, one per slot like the other per-solve buffers (overlapped: S + 1 needed)
    bool ticket_overlap = false;     // ticket path (deterministic kernel, K > 4096): consecutive launches of a batch overlap too (round 3)
    std::vector<float> dwa_stage;    // host staging of bn_mppi_dwa_solve's upload
    int *d_ticket = nullptr;
    float *d_gpart = nullptr;
    int n_cus = 256;
    size_t resident_wgs = 1024;      // role-kernel workgroups the device holds at once (LDS- and wave-limited) x CUs
    // overlapped launches: consecutive solves of one bn_mppi_solve_n_async call go round the handle's stream and n_streams - 1
    // extra ones; device counters carry the dependency (SolveParams.flag_part / flag_tail)
    int n_streams = 1;
    hipStream_t xstream[kMaxStreams - 1] = {};
    std::vector<hipStream_t> parked;            // streams that turned out to share the handle's hardware queue (see bn_mppi_create)
    hipEvent_t ev_fork = nullptr, ev_join[kMaxStreams - 1] = {};
    hipEvent_t ev_guard[kMaxStreams] = {};      // recorded on this handle's streams BY another handle that must run behind this one's overlapped batch
    unsigned long long *d_flags = nullptr;      // [kSlots][B] flag_part per slot and instance, [B] flag_tail per instance, then int err (accessors: mppi_launch.h)
    bool role_overlap = false;                  // the role kernel's launches of a batch may overlap too (see bn_mppi_solve_n_async)
    unsigned long long *d_gran[kSlots] = {};   // granule copies of the partial rows per slot (K <= 1024, 2T <= 320)
    // Second trajectory / control buffers for overlapped batches.  Two launches in flight must not write the same addresses: whose
    // dirty L2 lines reach memory last is decided by which KERNEL ends last, and a straggling aux workgroup can make the earlier
    // solve's kernel the later one to end (seen once per cold start: X / U of the last solve partly overwritten by its
    // predecessor's).  Solves of a batch go round n_streams buffers such that the LAST one writes the exposed buffer.
    float *d_Xalt[kMaxStreams - 1] = {}, *d_Ualt[kMaxStreams - 1] = {};
    unsigned long long pub[kSlots] = {};     // host mirror: what flag_part[slot][b] reaches once every launch issued so far has published
    unsigned long long tails = 0;               // host mirror of flag_tail[b]
    bool prev_published = false;                // the latest solve counted itself into flag_part (latency kernel): its successor may overlap
    bool overlap_used = false;                  // a wait could have expired since the last check of the error word
    bool overlap_off = false;                   // a wait DID expire once: this handle keeps to one stream from then on
    // The error word of the bounded device-side waits: pinned host memory the kernels write with a system-scope store, so every
    // entry point can look at it for free.  Journal: the batches enqueued since the word was last found clean at a
    // synchronisation point, with the mean the first of them started from (kept by that launch itself, SolveParams::mean_snap)
    // and the solve counter (= Philox position) at that point -- what recover_overlap() needs to run them again on one stream.
    int *h_err = nullptr, *d_err = nullptr;     // host address / device address of the same word
    unsigned long long *h_mail = nullptr, *d_mail = nullptr;   // (B, 2) granules {U*[0][d], solve index + 1}: see bn_mppi_first_action
    float *d_mean_snap = nullptr;
    float *d_state_snaps = nullptr;             // [snap_cap][B][3]: the states every journalled batch started from, kept by its first launch
    size_t snap_cap = 0;                        // (SolveParams::state_snap): a re-run reads these, not the caller's buffer
    size_t snap_slot = 0;                       // slot of the batch being enqueued
    bool arm_state_snap = false;                // the next launch fills it
    struct BatchRec { int32_t n; const float *states; const float *eps; bn_noise_kind noise; int32_t eps_ring; int64_t eps_stride; bool episode; const float *z; };
    std::vector<BatchRec> journal;
    bool journal_lost = false;                  // something not replayable happened since the last clean check (or too many batches)
    bool arm_snap = false;                      // the next launch keeps its mean in d_mean_snap
    bool replaying = false, last_batch_overlapped = false;
    uint64_t journal_solves0 = 0, recoveries = 0;
    // Self-protecting overlap (round 6).  Overlapped launches assume the device to themselves: with a co-tenant process on the GPU the
    // workgroups that wait for their predecessor hold slots the predecessor's stragglers need, and the chain runs at HALF the
    // one-stream rate (46 k against 80 k solves/s).  The handle watches its own cadence -- the first-action mailbox
    // counts finished solves, the host clock does the rest: no event, no kernel change -- over windows of 64 launches that found the
    // device backlogged at both ends, looks at the other mode once, and runs whichever is faster; it looks again when its cadence
    // degrades by half, and every 256 windows while it runs on one stream (has the co-tenant left?).
    struct OvTune { double best[2] = {0, 0}, last[2] = {0, 0}, ema[2] = {0, 0}; int chosen = 0, explore = 0, slow_run = 0; uint64_t windows[2] = {0, 0}, since_explore = 0, switches = 0; } tune;
    struct OvSample { bool valid = false; std::chrono::steady_clock::time_point t{}; uint32_t prog = 0, enq = 0; } ov_sample;
    int run_mode = 0;                // the mode of the batch being enqueued (0 overlapped, 1 one stream)
    // One launch per SYNCHRONOUS solve (round 6; bn_mppi_forward_async, bn_mppi_forward_state_async, bn_mppi_solve on the latency kernel):
    // the solve's own tail rides in its launch as a second aux workgroup (SolveParams::self_tail) -- no stand-alone finish kernel.
    float *self_out_copy = nullptr;  // the caller's U* | X* block of the forward() being enqueued (consumed by solve_impl)
    const float *inline_state = nullptr;   // host pointer: the state of the forward() being enqueued travels in the kernel arguments
    bool self_tail_launched = false; // the latest solve_impl call took the one-launch path (its tail is NOT pending)
    bool self_used = false;          // a self tail's bounded wait could have expired since the error word was last looked at
    bool self_off = false;           // ... and one did: two launches per synchronous solve from then on
    // Host-paced loop (BN_FLAG_HOST_PACED, round 6): bn_mppi_forward_state_async enqueues the NEXT solve's launch one control step ahead,
    // on one of two private streams; that launch waits on the device for the state the next call posts (rollout_lat.inc, HOSTP).
    bool hp_enabled = false;
    hipStream_t hp_stream[2] = {};   // [0] = xstream[0], [1] = xstream[1] (created for this mode); the launches alternate
    hipEvent_t hp_ev[2] = {};        // recorded behind every prelaunch; the handle's stream waits for it when the request is posted
    bool hp_unordered = false;       // BN_FLAG_UNORDERED_OUTPUTS: the handle's stream has not been ordered behind the latest posted solve yet ...
    int hp_unordered_q = 0;          // ... whose launch is the latest one on this private stream (see hp_order_now)
    unsigned long long *h_req = nullptr, *d_req = nullptr;         // pinned: kSlots x 8 request granules, then 16 status words (acknowledgements, "gave up" per slot)
    unsigned long long *req_bar = nullptr;                         // the request granules in DEVICE memory the host writes through the BAR (bar_alloc), or null
    unsigned long long *d_req_dev = nullptr;                       // device: kSlots x 8, republished by the launches' tail workgroups
    uint32_t hp_seq = 0;             // request tags, unique per prelaunch
    bool hp_armed = false;           // a prelaunched solve waits for its state
    uint32_t hp_tag = 0;             // ... its tag, request slot, stream index, trajectory buffer
    int hp_slot = 0, hp_q = 0, hp_xidx = 0;
    uint32_t hp_posted_tag = 0;      // the latest request posted (bn_mppi_first_action watches the give-up word for it)
    float hp_posted_state[3] = {};
    float *hp_posted_out = nullptr;
    bool hp_skip_check = false;      // test hook: post without looking whether the launch has given up (exercises the repair in bn_mppi_first_action)
    int hp_redo_q = -1;              // hp_redo: the private stream its solve runs on (the one the cancelled successor is not on), or -1
    float hp_prev_state[3] = {};     // the state of the latest forward (the next launch's speculative window is staged around it)
    bool hp_gran_valid = false;      // the latest solve published its partial rows as granules and nothing has touched the mean since
    int hp_extra = 2;                // cells the speculative window is wider on each side
    int x_idx = 0;                   // which trajectory / control buffer holds the latest solve (bn_mppi_states_buffer_index)
    int hp_next_q = 0;
    std::chrono::steady_clock::time_point hp_armed_at{};      // when the waiting launch was enqueued (a request is posted only well within its patience)
    int hp_polls = 25000;            // how long a prelaunched solve waits for its state: looks of ~2 us each (~50 ms); bn_mppi_debug_host_paced
    bool lat_kernel = false;         // plain pipelined solves of a launch that leaves every workgroup a CU: rollout_lat_kernel
    bool wave_kernel = false;        // plain pipelined solves use rollout_wave_kernel (episodes keep the role kernel)
    bool shard_pending = false;      // K-sharded solve: rollouts launched, tail waits for the partials of the other shards
    void *shard_comm = nullptr;      // ncclComm_t of bn_mppi_shard_comm_init: the exchange is enqueued by the library on the handle's stream
    int shard_world = 0, shard_rank = 0;
    bool shard_prepared = false;     // bn_mppi_shard_comm_prepare has run: buffers, events, side stream exist; the communicator may not yet
    bool shard_inplace = false;               // set around the rollouts of bn_mppi_shard_solve_async
    float *d_gathered = nullptr;     // (shard_world x nblk, 2 + 2T): every shard's partial rows, rank order
    float *d_shard_merged = nullptr; // kSlots x [U* (2T) then (max z, sum e)]: what the merge kernel hands to the tail on the side stream
    hipStream_t shard_side = nullptr;         // the tail of a library-enqueued sharded solve runs here, beside the next solve's rollouts
    bool shard_side_own = false;
    hipEvent_t ev_shard_merge = nullptr, ev_shard_tail[kSlots] = {};      // tail events by solve slot (see bn_mppi_shard_solve_async)
    int shard_tail_slot = 0;                  // slot of the latest tail
    bool shard_tail_inflight = false;         // the handle's stream has not been ordered behind the latest side-stream tail yet
    bool ticket_mode = false;        // one launch per solve: ticket merge by the last workgroup + the previous tail as aux
                                     // workgroup (sampled-slip kernel; deterministic kernel at K > 2048)
    bool slip_std_set = false;
    // device-side closed loop (bn_mppi_env_attach / bn_mppi_episode_async).  The three loops' logs: episode_log.h
    float *d_lat_mean = nullptr, *d_lat_std = nullptr, *d_env_state = nullptr;
    int *d_ep_done = nullptr;
    bool env_attached = false;
    bn::EpisodeLog ep_log;       // len: steps enqueued in the current episode
    const float *ep_z = nullptr; // (n_steps, B) device slip draws of the current episode, or nullptr
    bool in_episode = false;
    // fused A* + DWA episode (bn_astar_dwa_episode_async)
    int32_t *d_ad_i = nullptr;   // the loop's integer words (AdWords, mppi_loops.cpp)
    float *d_ad_state = nullptr; // (B, 3) the environment states the episode advances
    bn::EpisodeLog ad_log;       // + the sub-goals
    uint64_t ad_step = 0;        // episode steps since bn_astar_dwa_reset
    int ad_walk = 0;             // bn_astar_dwa_set_walk: 0 the serial next-hop walk, 1 the A* handle's jump tables
    // CL-RRT plan-follow-replan loop (bn_clrrt_loop_run)
    bn::ClrrtRover *d_cl_rover = nullptr;   // (B)
    int32_t *d_cl_flags = nullptr;          // the replan mask and the pending counter (ClFlags, mppi_loops.cpp)
    float *d_cl_goal = nullptr;             // (B, 3) goal nodes
    int32_t *d_cl_words = nullptr;          // what the latest run left of the rovers, by column (ClrrtOutcome, clrrt_view.h)
    bn::EpisodeLog cl_log;                  // + deviation, plan index, event
    int32_t *h_cl_pending = nullptr;        // pinned: the pending counter of the latest round
    hipEvent_t cl_ev[2] = {};               // around a follow launch (follow_ms)
    int32_t cl_iter = 0, cl_limit_steps = 0;   // iterations since the reset; the step count at which elapsed > time_limit
    bool cl_ready = false;                  // bn_clrrt_loop_reset has run
    bn_clrrt_t *cl_planner = nullptr;       // ... with this CL-RRT handle: the episode's goals, streams and paths live in it
    size_t scratch_bytes = 0, eps_bytes = 0, idx_count = 0;
    float *h_pinned = nullptr;   // pinned staging for (B,3) states
    // Who owns all of the above (bn_host.h): `bufs` is what bn_mppi_create allocates from its plan, plus d_scratch, d_eps and d_idx,
    // which grow on demand; the others are the groups a concern builds on first use and its *_release frees.  Streams are not in
    // any table.
    bn::DeviceBuffers bufs, env_bufs, ad_bufs, cl_bufs, shard_bufs, paced_bufs;
    size_t plan_bytes[BN_BUF_COUNT_] = {};   // MppiPlan::buffer_bytes: what bn_mppi_device_buffer reports for a buffer this handle does not have
    // launch log (bn_mppi_debug_launch_log): a ring of kLaunchLogCap records, allocated when recording is turned on
    bool log_on = false;
    std::vector<bn_mppi_launch_record> launch_log;
    uint64_t log_head = 0, log_read = 0;        // records made / handed out so far
    // profiling
    std::vector<hipEvent_t> ev;  // two-launch mode: 3 events per solve (start, after rollout, after finish);
    size_t ev_used = 0;          // pipelined mode: one event at the start of every group of kProfGroup launches
    int prof_in_group = 0;
};

// What more than one host file calls.  Hidden: nothing of this is an export of the library, and calls across the files bind directly.
namespace bn {
namespace host __attribute__((visibility("hidden"))) {

// mppi_capi.cpp
extern std::mutex g_overlap_mu;
extern std::map<int, std::vector<bn_mppi *>> g_handles;
extern std::map<int, bn_mppi *> g_overlap_owner;
extern std::atomic<int> g_overlap_owners;
int fail(int code, const char *fmt, ...);
int ensure_scratch(bn_mppi *h, size_t bytes);
int flush_tail(bn_mppi *h, float *out_copy = nullptr);
int check_instance(const bn_mppi *h, int32_t instance, bool allow_all);
void journal_arm_states(bn_mppi *h);
void journal_push(bn_mppi *h, bn_mppi::BatchRec r, bool replayable);
int self_check(bn_mppi *h);
int settle_point(bn_mppi *h);
void tune_record(bn_mppi *h, int mode, double us);
// mppi_solve.cpp.  solve_impl: `q` = the stream (and trajectory buffer) of a member of an overlapped batch, 0 = the handle's
int guard_foreign_overlap(bn_mppi *h);
int solve_impl(bn_mppi_t *h, const float *states, bn_mem_kind states_where, const float *eps, bn_noise_kind noise,
               bool shard_rollout, bool overlap = false, int q = 0, bool self_tail = false);
// each concern frees what it allocates (bn_mppi_destroy calls them); paced_setup is bn_mppi_create's host-paced part
int paced_setup(bn_mppi *h, bool may_overlap);      // mppi_paced.cpp
void paced_release(bn_mppi *h);
void shard_comm_release(bn_mppi *h);                // mppi_shard.cpp
void env_release(bn_mppi *h);                       // mppi_env.cpp
void loops_release(bn_mppi *h);                     // mppi_loops.cpp

}  // namespace host
}  // namespace bn

#define BN_HIP(expr)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            (void)hipGetLastError();   /* reported here: do not leave it for the next HIP user of the process (torch) */ \
            return fail(BN_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),  \
                        __FILE__, __LINE__);                                                 \
        }                                                                                    \
    } while (0)

namespace {

// What the buffer tables report through (bn_host.h).  The sticky HIP error is taken here: reported through the return code, it must
// not surface in the caller's next torch call.
static inline int table_fail(int code, const std::string &msg)
{
    if (code == BN_ERR_HIP) (void)hipGetLastError();
    return bn::host::fail(code, "%s", msg.c_str());
}

// After a group was built or a buffer grew outside bn_mppi_create: the tables' zero fills run on the null stream, and a private
// handle stream is not ordered behind that one (seen: a fill landing on top of what the handle's stream had just written).
static inline int fills_done()
{
    return hipStreamSynchronize(nullptr) == hipSuccess ? BN_OK : table_fail(BN_ERR_HIP, "hipStreamSynchronize failed behind an allocation");
}

// Every entry point works on the handle's device and leaves the calling thread's current device as it found it
// (one process may drive several GPUs; torch tracks its own notion of the current device).
using bn::DeviceGuard;                      // bn_host.h
#define BN_BIND_Q(h) DeviceGuard bn_guard_((h)->cfg.device_id); if (!bn_guard_.ok) return fail(BN_ERR_HIP, "hipSetDevice failed")

// BN_FLAG_UNORDERED_OUTPUTS: the host-paced forward left the handle's stream unordered behind the latest posted solve (a stream-wait on a
// pending event is 3-5 us of host time per control step, for consumers that mostly are not there).  Every entry point that enqueues on the
// handle's stream or hands out results makes up for it here, once -- everything except the loop's own two calls.
static inline void hp_order_now(bn_mppi *h)
{
    if (!h->hp_unordered) return;
    h->hp_unordered = false;
    if (hipStreamWaitEvent(h->stream, h->hp_ev[h->hp_unordered_q], 0) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(h->hp_stream[h->hp_unordered_q]);
    }
}
#define BN_BIND(h) BN_BIND_Q(h); hp_order_now(h)

// ---- host-paced loop: the request words --------------------------------------------------------------------------------------
// A request is six {value, tag} granules in pinned memory (x, y, theta, the caller's output block lo / hi, the command); the
// launch's tail workgroup takes them when all six carry the launch's tag.  Plain 8-byte stores: x86 keeps them in order, and each
// granule vouches for itself anyway.
static inline void hp_write_request(bn_mppi *h, int slot, uint32_t tag, const float st[3], const float *out, uint32_t cmd)
{
    unsigned long long *r = (h->req_bar ? h->req_bar : h->h_req) + (size_t)slot * 8;
    uint32_t w[6] = {0, 0, 0, 0, 0, cmd};
    if (st) std::memcpy(w, st, 12);
    const unsigned long long o = (unsigned long long)(uintptr_t)out;
    w[3] = (uint32_t)o; w[4] = (uint32_t)(o >> 32);
    for (int i = 0; i < 6; ++i) __atomic_store_n(r + i, ((unsigned long long)tag << 32) | w[i], __ATOMIC_RELEASE);
    if (h->req_bar) __builtin_ia32_sfence();           // device memory through the BAR is write-combining: out with it now
}

// The tail workgroup of the launch with this tag gave up waiting for the host (~50 ms) and said so: the launch has ended, nothing happened.
static inline bool hp_gave_up(const bn_mppi *h, uint32_t tag)
{
    return tag != 0 && h->h_req && __atomic_load_n(h->h_req + (size_t)kSlots * 8 + 8 + (tag % kSlots), __ATOMIC_ACQUIRE) == (((unsigned long long)tag << 32) | 2ull);
}

// A launch that still waits for its state is told to leave -- it has touched nothing but its own LDS -- and the host's bookkeeping
// goes back to where it was before the prelaunch: exactly what hp_prelaunch (mppi_paced.cpp) advanced through advance_mirrors
// (mppi_launch.h) -- nblk published into the solve's slot, one tail -- and the solve counter.  No synchronisation: the launch ends by
// itself within a poll.
static inline void hp_cancel(bn_mppi *h)
{
    if (!h->hp_armed) return;
    hp_write_request(h, h->hp_slot, h->hp_tag, nullptr, nullptr, 2u);
    h->hp_armed = false;
    h->solves -= 1;
    const int cur3 = (int)(h->solves % kSlots);
    h->pub[cur3] -= (unsigned long long)h->p.nblk;
    h->tails -= 1;
    h->hp_next_q = h->hp_q;                            // (the stream the cancelled launch leaves within a poll)
}

}  // namespace
