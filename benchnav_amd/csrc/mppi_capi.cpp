// mppi_capi.cpp -- host side of the C ABI declared in include/benchnav_mppi.h: the core.
//
// Owns the device buffers of one planner handle (mppi_handle.h) and enqueues the two kernels of
// a solve (mppi_kernels.hip) on the handle's HIP stream.  No torch types, no CPU
// fallback: creation fails without a gfx950 device.
//
// Here: the error string, the per-device overlap ownership, the journal and the recovery of expired waits, the stand-alone tail,
// create (from the plan of mppi_plan.cpp: register the buffers, allocate, probe) / destroy / setters, the tuner, sync / flush.  The other
// concerns have a file each: mppi_solve.cpp (everything a solve executes: solve_impl, bn_mppi_solve_n_async, on the launch decision of
// mppi_launch.h), mppi_paced.cpp (host-paced loop, forward), mppi_shard.cpp (K-shard exchange), mppi_env.cpp (closed-loop
// environment, DWA), mppi_loops.cpp (A*+DWA and CL-RRT loops), mppi_query.cpp (getters, profiling, lab hooks).
#include "mppi_plan.h"
#include "mppi_launch.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

namespace bn {
namespace host {

static thread_local std::string g_last_error;

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

// One overlapped batch per device at a time.  Workgroups of an overlapped launch hold their slots while they wait for their
// predecessor; two handles doing that at once can starve each other's predecessors of slots until the bounded waits expire
// (8 handles x 8 instances: seen).  A handle overlaps only while no OTHER handle's overlapped batch is still in flight on its
// device (its streams still busy); otherwise this batch runs in one stream, which is always safe.
std::mutex g_overlap_mu;
std::map<int, bn_mppi *> g_overlap_owner;   // device -> the handle whose overlapped batch was enqueued last
// ... and nothing ELSE of this process beside it (round 4).  The rule above kept two overlapped batches apart; a differential sweep
// over pairs of planners (tools/fuzz_features2.py) still saw waits expire: one planner's overlapped batch of latency-kernel
// launches -- one workgroup per CU, sized for a device it has to itself -- with the other planner's ordinary one-stream launches
// in between (12 % of the runs of one pattern, depending on the order the handles' queues were created in).  So a batch
// overlaps only while EVERY other handle on the device is idle (g_handles), and a launch of another handle that arrives while an
// overlapped batch is in flight is ordered behind that batch's end by events (order_behind_foreign_overlap): no host blocking,
// the kernels simply do not share the device with waiting workgroups.
std::map<int, std::vector<bn_mppi *>> g_handles;   // device -> live handles (guarded by g_overlap_mu)
std::atomic<int> g_overlap_owners{0};              // devices with an owner: the launch path looks at it without the lock
// (... and one PROCESS per device for launches big enough to crowd each other out: own_device_for_big_overlap, mppi_solve.cpp)

int ensure_scratch(bn_mppi *h, size_t bytes)
{
    if (bytes <= h->scratch_bytes) return BN_OK;
    h->scratch_bytes = 0;
    if (int rc = h->bufs.resize(&h->d_scratch, bytes, table_fail)) return rc;
    h->scratch_bytes = bytes;
    return fills_done();
}

// Write the tail (U*, next mean, X*, weights, cost copy) of the latest solve if it is still pending.
int flush_tail(bn_mppi *h, float *out_copy)
{
    if (h->shard_tail_inflight) {                      // K-sharded solve, library-enqueued: results are ordered on the handle's stream from here on
        BN_HIP(hipStreamWaitEvent(h->stream, h->ev_shard_tail[h->shard_tail_slot], 0));
        h->shard_tail_inflight = false;
    }
    if (!h->tail_pending) return BN_OK;
    bn::SolveParams p = h->p;
    p.out_copy = out_copy;
    const int cur3 = (int)((h->solves - 1) % kSlots);
    p.part = h->d_part[cur3]; p.cost = h->d_cost[cur3]; p.state = h->d_state_copy[cur3];
    if (h->ticket_mode) {
        p.tail_merged = 1;
        p.ustar_prev = h->d_ustar2[cur3]; p.stats_prev = h->d_stats2[cur3];
    }
    p.tail_solve = h->solves - 1;
    if (h->in_episode) {
        p.env_on = 1;
        p.ep_index = h->ep_log.len - 1;
        p.env_z = h->ep_z ? h->ep_z + (size_t)(h->ep_log.len - 1) * p.B : nullptr;
    }
    p.flag_tail = flag_tail(h);                        // every tail counts itself in (stream-ordered here: nothing to wait for)
    h->tails += 1;
    if (h->overlap_used) p.err_dev = err_dev(h);       // behind overlapped launches: see raise_wait_expired
    if (int rc = guard_foreign_overlap(h)) return rc;
    if (h->log_on) {
        bn_mppi_launch_record r{};
        r.call = kCallTail; r.entry = kFinish; r.u_buf = p.U ? 0 : -1; r.flag_tail = 1;
        r.tail_merged = p.tail_merged; r.tail_solve = p.tail_solve; r.env_on = p.env_on; r.ep_index = p.ep_index;
        r.env_z = p.env_z != nullptr; r.err_dev = p.err_dev != nullptr;
        log_launch(h, r);
    }
    BN_HIP(bn::launch_finish(p, h->stream));
    h->tail_pending = false;
    return BN_OK;
}

int check_instance(const bn_mppi *h, int32_t instance, bool allow_all)
{
    if (!h) return fail(BN_ERR_INVALID, "null handle");
    if (instance == -1 && allow_all) return BN_OK;
    if (instance < 0 || instance >= h->p.B)
        return fail(BN_ERR_INVALID, "instance %d out of range [0,%d)", instance, h->p.B);
    return BN_OK;
}

// Called before the first launch of a batch that journal_push may record: that launch copies the states it reads into the slot
// the record will point at.  (Costs nothing on the host; one predicated 12-byte store in the kernel.)
void journal_arm_states(bn_mppi *h)
{
    if (h->replaying) return;
    h->snap_slot = h->journal.size();
    h->arm_state_snap = h->snap_slot < h->snap_cap;
}

void journal_push(bn_mppi *h, bn_mppi::BatchRec r, bool replayable)
{
    if (h->replaying) return;
    if (!h->last_batch_overlapped && h->journal.empty()) return;      // nothing in flight that a wait could have spoilt
    if (!replayable || h->journal.size() >= std::min(kJournalCap, h->snap_cap) || h->snap_slot != h->journal.size()) { h->journal_lost = true; h->journal.clear(); return; }
    r.states = h->d_state_snaps + h->snap_slot * (size_t)h->p.B * 3;  // what the batch's first launch kept (journal_arm_states)
    if (!h->journal_lost) h->journal.push_back(r);
}

// A bounded device-side wait of an overlapped launch expired: that launch computed on incomplete partials, and every solve
// warm-started from it since is invalid as well.  Bring the handle to rest, forget the counters, and run the journalled batches
// again on ONE stream from the mean the first of them started from: same inputs (the states each batch's first launch kept in
// d_state_snaps; the callers' noise buffers, which must stay valid until the synchronisation point that follows a batch, as for
// any asynchronous call), same Philox positions, hence
// the results the overlapped launches would have produced.  The handle keeps to one stream from then on: whatever kept a
// predecessor from becoming resident (another process on the GPU, most likely) may still be there.
// BN_OK with a warning in bn_last_error() when the re-run succeeded (bn_mppi_recovery_count counts them: consumers enqueued
// in stream order BEFORE this synchronisation point have read invalid buffers); BN_ERR_HIP when there was nothing to re-run from.
static int recover_overlap(bn_mppi *h)
{
    for (int q = 0; q < kMaxStreams - 1; ++q)
        if (h->xstream[q]) BN_HIP(hipStreamSynchronize(h->xstream[q]));
    BN_HIP(hipStreamSynchronize(h->stream));
    BN_HIP(hipMemset(h->d_flags, 0, flag_bytes(h->p.B)));      // counters and the device error word
    // ... and the ticket counters of the ticket merge (K > 4096, sampled slip): they are per instance, not per launch -- a launch that
    // gave up waiting and the starved predecessor it gave up on draw from them at the same time, and the merger's reset to zero races
    // with the other launch's increments.  Left non-zero they make the re-run's first launch merge before its rows are complete: a
    // repair with wrong results (round 4, tests/differential.py `ops` seed 2681: half of the natural expiries of that configuration).
    if (h->d_ticket) BN_HIP(hipMemset(h->d_ticket, 0, (size_t)h->p.B * 65 * 4));
    for (int q = 0; q < kSlots; ++q) h->pub[q] = 0;
    h->tails = 0;
    h->prev_published = false;
    h->tail_pending = false;
#ifdef BN_EXPERIMENTS
    fprintf(stderr, "[bn] expired wait: counter %d (B=%d: [slot][b] below %d, tails above) need %d seen %d | solve %d block (%d,%d) have_prev/overlap/cur_slot %d wait_part*1000+wait_tail %d | host: solves %llu tails %llu pub %llu %llu %llu %llu\n",
            h->h_err[8], h->p.B, kSlots * h->p.B, h->h_err[9], h->h_err[10], h->h_err[11], h->h_err[12], h->h_err[13], h->h_err[14], h->h_err[15],
            (unsigned long long)h->solves, (unsigned long long)h->tails, (unsigned long long)h->pub[0], (unsigned long long)h->pub[1], (unsigned long long)h->pub[2], (unsigned long long)h->pub[kSlots - 1]);
#endif
    h->overlap_off = true;
    h->overlap_used = false;
    h->arm_snap = false;
    h->arm_state_snap = false;
    h->in_episode = false;
    *h->h_err = 0;
    std::vector<bn_mppi::BatchRec> recs;
    recs.swap(h->journal);
    const bool lost = h->journal_lost || recs.empty();
    h->journal_lost = false;
    if (lost)
        return fail(BN_ERR_HIP, "an overlapped launch gave up waiting for its predecessor's partials and the batches since the last "
                                "synchronisation point cannot be re-run: their results are invalid; this handle runs its launches on one "
                                "stream from now on");
    BN_HIP(hipMemcpy(h->d_mean, h->d_mean_snap, (size_t)h->p.B * h->p.T * 2 * 4, hipMemcpyDeviceToDevice));
    h->solves = h->journal_solves0;
    h->replaying = true;
    int rc = BN_OK;
    for (const auto &r : recs) {
        rc = r.episode ? bn_mppi_episode_async(h, r.n, r.states, BN_MEM_DEVICE, r.eps, r.noise, r.eps_ring, r.eps_stride, r.z)
                       : bn_mppi_solve_n_async(h, r.n, r.states, BN_MEM_DEVICE, r.eps, r.noise, r.eps_ring, r.eps_stride);
        if (rc != BN_OK) break;
    }
    if (rc == BN_OK) rc = flush_tail(h);
    h->replaying = false;
    if (rc != BN_OK) return rc;
    BN_HIP(hipStreamSynchronize(h->stream));
    h->recoveries += 1;
    (void)fail(BN_OK, "warning: an overlapped launch gave up waiting for its predecessor's partials; %zu batch(es) were re-run on one "
                      "stream (results are valid now; this handle no longer overlaps its launches)", recs.size());
    return BN_OK;
}

// The handle's stream has just been synchronised (`synced`), or the caller only wants to know what has ALREADY gone wrong:
// look at the error word, repair if it is set.
static int settle_overlap(bn_mppi *h, bool synced)
{
    if (!h->overlap_used || h->replaying) return BN_OK;
    if (__atomic_load_n(h->h_err, __ATOMIC_ACQUIRE) == 0) {
        if (synced) {
            bool idle = true;                                  // the extra streams are joined into the handle's stream; make sure
            for (int q = 0; idle && q + 1 < h->n_streams; ++q) idle = hipStreamQuery(h->xstream[q]) == hipSuccess;
            (void)hipGetLastError();
            if (idle) { h->overlap_used = false; h->journal.clear(); h->journal_lost = false; }
        }
        return BN_OK;
    }
    return recover_overlap(h);
}

static int sync_checked(bn_mppi *h)
{
    BN_HIP(hipStreamSynchronize(h->stream));
    // the extra streams of an overlapped batch are not joined into the handle's stream (see bn_mppi_solve_n_async): their last
    // kernels have done all their work by now -- the handle's stream consumed it -- and end within microseconds
    if (h->overlap_used)
        for (int q = 0; q + 1 < h->n_streams; ++q)
            if (h->xstream[q]) BN_HIP(hipStreamSynchronize(h->xstream[q]));
    return settle_overlap(h, true);
}

// The tail of a one-launch synchronous solve waits (bounded) for the rollout workgroups of its OWN launch.  They are dispatched before
// it and wait for nobody, so the wait ends -- as surely as a barrier does; should it ever expire (the error word, looked at here for
// free) the latest solve's outputs are invalid and there is nothing to re-run from: report it, and keep to two launches from then on.
int self_check(bn_mppi *h)
{
    if (!h->self_used || h->overlap_used || h->replaying) return BN_OK;      // (behind overlapped batches: settle_overlap looks at the same word)
    if (__atomic_load_n(h->h_err, __ATOMIC_ACQUIRE) == 0) return BN_OK;
    BN_HIP(hipStreamSynchronize(h->stream));
    BN_HIP(hipMemset(h->d_flags, 0, flag_bytes(h->p.B)));
    for (int q = 0; q < kSlots; ++q) h->pub[q] = 0;
    h->tails = 0;
    *h->h_err = 0;
    h->self_used = false;
    h->self_off = true;
    return fail(BN_ERR_HIP, "the tail of a one-launch solve gave up waiting for the rollout workgroups of its own launch: the outputs of solve %llu "
                            "are invalid (solve again); this handle goes back to two launches per synchronous solve",
                (unsigned long long)h->solves - 1);
}

// Entry points that hand results to the host, change the planner's inputs, or enqueue work the journal does not describe: whatever
// an expired wait could have spoilt is repaired first.  Free unless overlapped launches are outstanding (then: one synchronisation).
int settle_point(bn_mppi *h)
{
    hp_cancel(h);                                      // (a launch waiting for the host's next state: this call is not that state)
    h->hp_gran_valid = false;
    if (int rc = self_check(h)) return rc;
    if (!h->overlap_used || h->replaying) return BN_OK;
    if (int rc = flush_tail(h)) return rc;
    return sync_checked(h);
}

void tune_record(bn_mppi *h, int mode, double us)
{
    bn_mppi::OvTune &t = h->tune;
    t.last[mode] = us;
    t.ema[mode] = t.ema[mode] == 0 ? us : t.ema[mode] + (us - t.ema[mode]) / 8;
    // the mode's best cadence: the minimum over windows that are not implausibly fast (one short window -- a host hiccup between two
    // looks at the mailbox -- must not become the yardstick everything after it fails)
    if (us >= 0.7 * t.ema[mode] && (t.best[mode] == 0 || us < t.best[mode])) t.best[mode] = us;
    t.windows[mode] += 1;
    if (mode == t.chosen) {
        t.since_explore += 1;
        t.slow_run = (t.best[mode] > 0 && us > 1.5 * t.best[mode]) ? t.slow_run + 1 : 0;
        if (t.chosen == 0) {
            if (t.best[1] == 0) { if (t.windows[0] >= 64) { t.explore = 1; t.since_explore = 0; } }      // never seen the other mode: look once (4096 launches in)
            else if (t.slow_run >= 4) {                    // four windows in a row at 1.5 x this mode's best: somebody else is on the device
                t.slow_run = 0;
                if (us > 1.15 * t.best[1]) { t.chosen = 1; t.switches += 1; t.since_explore = 0; }   // ... and one stream was faster than this when last seen
                else if (t.since_explore >= 64) { t.explore = 1; t.since_explore = 0; }
            }
        } else if (t.since_explore >= 256) { t.explore = 1; t.since_explore = 0; }                 // has the co-tenant left?
    } else {                                           // a look at the other mode
        if (t.last[t.chosen] > 0 && us < 0.9 * t.last[t.chosen]) { t.chosen = mode; t.switches += 1; t.since_explore = 0; t.slow_run = 0; }
        t.explore = 0;
    }
}

}  // namespace host
}  // namespace bn

using namespace bn::host;

extern "C" {

void bn_mppi_config_init(bn_mppi_config *c)
{
    std::memset(c, 0, sizeof *c);
    c->struct_size = sizeof *c;
    c->horizon = 50;
    c->num_samples = 1024;
    c->num_instances = 1;
    c->grid_size = 64;
    c->resolution = 0.5f;
    c->x_limits[0] = c->y_limits[0] = 0.0f;
    c->x_limits[1] = c->y_limits[1] = 32.0f;
    c->sigma[0] = c->sigma[1] = 0.5f;
    c->inv_var[0] = c->inv_var[1] = 4.0f;
    c->lambda_ = 0.5f;
    c->u_min[0] = 0.0f; c->u_min[1] = -1.0f;
    c->u_max[0] = 1.0f; c->u_max[1] = 1.0f;
    c->dt = 0.1f;
    c->stuck_threshold = 0.3f;
    c->seed = 42;
}

// Everything bn_mppi_create allocates, entered into the handle's table from the plan: in the order, and under the conditions, the
// handle has always allocated it.  The sizes of the buffers bn_mppi_device_buffer hands out are the plan's.
static void register_buffers(bn_mppi *h, const MppiPlan &m)
{
    const bn::SolveParams &p = h->p;
    const size_t B = p.B, K = p.K, T = p.T;
    const uint64_t *pub = m.buffer_bytes;
    bn::DeviceBuffers &t = h->bufs;
    t.add(&h->d_map, pub[BN_BUF_MAP], BN_BUF_MAP);
    t.add(&h->d_state, B * 3 * 4);
    t.add(&h->d_goal, pub[BN_BUF_GOAL], BN_BUF_GOAL);
    t.add(&h->d_mean, pub[BN_BUF_MEAN], BN_BUF_MEAN);
    if (m.has_X) t.add(&h->d_X, pub[BN_BUF_STATES], BN_BUF_STATES);
    t.add(&h->d_mean_used, B * T * 2 * 4);
    if (m.has_U) t.add(&h->d_U, pub[BN_BUF_CONTROLS], BN_BUF_CONTROLS);
    for (int q = 0; q < kSlots; ++q) {
        t.add(&h->d_cost[q], B * K * 4);
        t.add(&h->d_part[q], B * (size_t)p.nblk * (2 + 2 * T) * 4);
        t.add(&h->d_state_copy[q], B * 3 * 4);
    }
    t.add(&h->d_cost_out, pub[BN_BUF_COSTS], BN_BUF_COSTS);
    t.add(&h->d_w, pub[BN_BUF_WEIGHTS], BN_BUF_WEIGHTS);
    t.add(&h->d_ustar, pub[BN_BUF_USTAR_XSTAR], BN_BUF_USTAR_XSTAR);   // U* then X* in ONE block: a caller copies both at once
    t.add(&h->d_stats, B * 2 * 4);
    t.add_pinned(&h->h_pinned, B * 3 * 4);
    t.add(&h->d_flags, flag_bytes(B));                 // [kSlots][B] + [B] counters, a spare slot, the device error word (mppi_launch.h)
    t.add(&h->d_mean_snap, B * T * 2 * 4);
    t.add_pinned(&h->h_err, 64, hipHostMallocMapped);
    t.add_pinned(&h->h_mail, B * 2 * sizeof(unsigned long long), hipHostMallocMapped);
    if (m.has_granules)
        for (int q = 0; q < kSlots; ++q) t.add(&h->d_gran[q], (B * (size_t)p.nblk * (2 + 2 * T) + 4 * B) * sizeof(unsigned long long));   // rows, then 4 per instance for the state
    if (m.has_alt) {
        for (int q = 0; q + 1 < m.n_streams; ++q) {
            if (m.has_X) t.add(&h->d_Xalt[q], pub[BN_BUF_STATES], q ? -1 : BN_BUF_STATES_ALT);
            if (m.has_U) t.add(&h->d_Ualt[q], pub[BN_BUF_CONTROLS], q ? -1 : BN_BUF_CONTROLS_ALT);
        }
        t.add(&h->d_state_snaps, m.snap_cap * B * 3 * 4);      // the journal's state snapshots: only a handle that can overlap ever journals
        t.add_event(&h->ev_fork, hipEventDisableTiming);
        for (int q = 0; q < m.n_streams; ++q) t.add_event(&h->ev_guard[q], hipEventDisableTiming);
        for (int q = 0; q + 1 < m.n_streams; ++q) t.add_event(&h->ev_join[q], hipEventDisableTiming);
    }
    if (m.has_slip_std) t.add(&h->d_slip_std, pub[BN_BUF_MAP]);
    if (m.has_ticket_buffers) {
        for (int q = 0; q < kSlots; ++q) {
            t.add(&h->d_ustar2[q], B * T * 2 * 4);
            t.add(&h->d_stats2[q], B * 2 * 4);
        }
        t.add(&h->d_ticket, B * 65 * 4);
        t.add(&h->d_gpart, B * 64 * (2 + 2 * T) * 4);
    }
    t.add_later(&h->d_scratch);
    t.add_later(&h->d_eps);
    t.add_later(&h->d_idx);
}

// The handle's stream (the caller's, or a private one) and the extra streams of overlapped launches.
static int open_streams(bn_mppi *h)
{
    if (!(h->cfg.flags & BN_FLAG_PRIVATE_STREAM)) h->stream = (hipStream_t)h->cfg.stream;          // may be the null stream
    else if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) == hipSuccess) h->own_stream = true;
    else return fail(BN_ERR_HIP, "hipStreamCreate failed");
    for (int q = 0; q + 1 < h->n_streams; ++q)
        if (hipStreamCreateWithFlags(&h->xstream[q], hipStreamNonBlocking) != hipSuccess)
            return fail(BN_ERR_HIP, "stream / event creation for overlapped launches failed");
    return BN_OK;
}

// General resolution: the in-loop lookups divide with the three-instruction quotient (quotient_general); check it over every
// float they can see -- ~1e9 values, a millisecond -- before anything relies on it.
static int check_quotient(bn_mppi *h)
{
    bn::SolveParams &p = h->p;
    if (p.pow2) return BN_OK;
    int rc = BN_OK;
    unsigned long long *bad = spare_counter(h);        // zero
    const float d_max = std::max(p.x_hi - p.x0, p.y_hi - p.y0);
    unsigned long long n_bad = 1;
    if (!(std::isfinite(d_max) && d_max >= 0.0f) || bn::launch_quotient_check(p.res, p.inv_res, d_max, bad, nullptr) != hipSuccess ||
        hipMemcpy(&n_bad, bad, sizeof n_bad, hipMemcpyDeviceToHost) != hipSuccess) {
        (void)hipGetLastError();
        rc = fail(BN_ERR_HIP, "checking the cell-index quotient for resolution %g failed", (double)p.res);
    } else if (n_bad != 0) {
        rc = fail(BN_ERR_INVALID, "resolution %.9g: the correctly rounded three-instruction quotient disagrees with the division for %llu "
                                  "positions in [0, %g] (no such resolution was known: please report it); use a neighbouring value",
                  (double)p.res, n_bad, (double)d_max);
    } else {
        p.fast_div = 1;
    }
    (void)hipMemset(bad, 0, sizeof n_bad);
    return rc;
}

// Overlapped launches need an extra stream that DISPATCHES concurrently with the handle's stream.  HIP deals its streams onto a
// handful of hardware queues in creation order, so which queue a fresh stream lands on depends on how many streams the process
// has created before: a process that brought up RCCL first got the handle's own queue (15.2 instead of 9.6 us per solve: no
// overlap at all).  Ask the hardware (launch_queue_probe: can the candidate dispatch while a grid larger than the chip is still
// being placed on the handle's stream?); a candidate that fails is parked and a fresh stream takes its place.
static int probe_overlap_streams(bn_mppi *h)
{
    if (h->n_streams < 2) return BN_OK;                // (a handle that never overlaps)
    int rc = BN_OK;
    int *probe = reinterpret_cast<int *>(spare_counter(h));
    for (int q = 0; rc == BN_OK && q + 1 < h->n_streams; ++q) {
        bool found = false;
        for (int attempt = 0; attempt < 8; ++attempt) {
            int seen = 0;
            if (hipMemset(probe, 0, 2 * sizeof(int)) != hipSuccess || bn::launch_queue_probe(probe, h->stream, h->xstream[q], h->n_cus) != hipSuccess ||
                hipStreamSynchronize(h->stream) != hipSuccess || hipStreamSynchronize(h->xstream[q]) != hipSuccess ||
                hipMemcpy(&seen, probe + 1, sizeof seen, hipMemcpyDeviceToHost) != hipSuccess) {
                (void)hipGetLastError();
                rc = fail(BN_ERR_HIP, "probing the streams of overlapped launches failed");
                break;
            }
            if (seen) { found = true; break; }
            if (attempt == 7) break;                   // (the stream in hand has been probed and failed: do not swap it for an unprobed one)
            hipStream_t fresh = nullptr;
            if (hipStreamCreateWithFlags(&fresh, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); break; }
            h->parked.push_back(h->xstream[q]);        // kept alive until destroy: destroying it would hand its queue slot to the next one
            h->xstream[q] = fresh;
        }
        if (exp_env("BN_DEBUG_CREATE")) std::fprintf(stderr, "[bn_mppi_create] extra stream %d: %s after %zu replacement(s)\n", q, found ? "dispatches concurrently" : "NO concurrent queue found", h->parked.size());
        // No stream that dispatches concurrently with the handle's: launches of a batch would not overlap, and workgroups waiting
        // on the device for a predecessor the queue has not started yet would only burn their bounded waits.  One stream then.
        if (!found && rc == BN_OK) h->overlap_off = true;
    }
    (void)hipMemset(probe, 0, 2 * sizeof(int));
    return rc;
}

// Plan (mppi_plan.h: every check and decision, no device), open the device, allocate what the plan lists, then the two questions
// only the device answers: the quotient check and the queue probe.
int bn_mppi_create(const bn_mppi_config *cfg, bn_mppi_t **out)
{
    if (!cfg || !out) return fail(BN_ERR_INVALID, "null argument");
    *out = nullptr;
    // (the CU count enters the plan; a configuration the plan refuses is refused before the device is looked at, as ever)
    MppiPlan plan{};
    if (int rc = plan_mppi(*cfg, 256, &plan)) return rc;
    if (int rc = bn::open_device(cfg->device_id, table_fail)) return rc;
    DeviceGuard guard(cfg->device_id);
    if (!guard.ok) return fail(BN_ERR_HIP, "hipSetDevice(%d) failed", cfg->device_id);
    hipDeviceProp_t prop;
    BN_HIP(hipGetDeviceProperties(&prop, cfg->device_id));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(BN_ERR_NO_DEVICE, "device %d is %s; this library is built for gfx950 only", cfg->device_id,
                    prop.gcnArchName);
    if (int rc = plan_mppi(*cfg, prop.multiProcessorCount, &plan)) return rc;

    bn_mppi *h = new bn_mppi();
    h->cfg = *cfg;
    h->p = plan.p;
    h->n_cus = plan.n_cus; h->n_maps = plan.n_maps; h->resident_wgs = plan.resident_wgs;
    h->slow_path = plan.slow_path; h->pipelined = plan.pipelined; h->wave_kernel = plan.wave_kernel; h->lat_kernel = plan.lat_kernel;
    h->role_overlap = plan.role_overlap; h->ticket_overlap = plan.ticket_overlap; h->ticket_mode = plan.ticket_mode;
    h->n_streams = plan.n_streams; h->snap_cap = plan.snap_cap;
    std::copy(plan.buffer_bytes, plan.buffer_bytes + BN_BUF_COUNT_, h->plan_bytes);
    register_buffers(h, plan);
    int rc = h->bufs.alloc_all(table_fail);
    if (rc == BN_OK && (hipHostGetDevicePointer((void **)&h->d_err, h->h_err, 0) != hipSuccess ||
                        hipHostGetDevicePointer((void **)&h->d_mail, h->h_mail, 0) != hipSuccess))
        rc = table_fail(BN_ERR_HIP, "hipHostGetDevicePointer failed");
    if (rc == BN_OK) rc = open_streams(h);
    if (rc == BN_OK) {
        bn::SolveParams &p = h->p;
        h->d_xstar = h->d_ustar + (size_t)p.B * p.T * 2;
        p.map = h->d_map; p.state = h->d_state; p.goal = h->d_goal; p.mean = h->d_mean; p.eps = nullptr;
        p.X = h->d_X; p.U = h->d_U; p.cost = h->d_cost[0]; p.part = h->d_part[0]; p.w = h->d_w;
        p.state_copy = h->d_state_copy[0]; p.cost_out = h->d_cost_out;
        p.ustar = h->d_ustar; p.xstar = h->d_xstar; p.stats = h->d_stats; p.mean_used = h->d_mean_used;
        p.mail = h->d_mail;
        p.slip_std = h->d_slip_std; p.gpart = h->d_gpart;
        if (p.slip_on) p.ticket = h->d_ticket;         // (p.ticket stays null in the deterministic kernel's h->p: only the one-launch path selects the ticket kernel)
        rc = check_quotient(h);
    }
    if (rc == BN_OK && hipDeviceSynchronize() != hipSuccess) rc = fail(BN_ERR_HIP, "hipDeviceSynchronize failed after allocation");
    if (rc == BN_OK) rc = probe_overlap_streams(h);
    // Host-paced loop (BN_FLAG_HOST_PACED): a second private stream that dispatches concurrently with the first, the request words, events
    if (rc == BN_OK) rc = paced_setup(h, plan.may_overlap);
    if (rc != BN_OK) {
        bn_mppi_destroy(h);
        return rc;
    }
    {
        std::lock_guard<std::mutex> lock(g_overlap_mu);
        g_handles[h->cfg.device_id].push_back(h);
    }
    *out = h;
    return BN_OK;
}

void bn_mppi_destroy(bn_mppi_t *h)
{
    if (!h) return;
    DeviceGuard guard(h->cfg.device_id);
    hp_cancel(h);
    (void)hipStreamSynchronize(h->stream);
    {
        std::lock_guard<std::mutex> lock(g_overlap_mu);
        auto it = g_overlap_owner.find(h->cfg.device_id);
        if (it != g_overlap_owner.end() && it->second == h) g_overlap_owner.erase(it);
        g_overlap_owners.store((int)g_overlap_owner.size(), std::memory_order_relaxed);
        auto &v = g_handles[h->cfg.device_id];
        v.erase(std::remove(v.begin(), v.end(), h), v.end());
    }
    for (hipEvent_t e : h->ev) (void)hipEventDestroy(e);
    if (h->shard_comm || h->shard_prepared) shard_comm_release(h);
    env_release(h);
    loops_release(h);
    paced_release(h);
    h->bufs.free_all();                                // what bn_mppi_create and the solve path allocated
    for (hipStream_t &xs : h->xstream)
        if (xs) { (void)hipStreamSynchronize(xs); (void)hipStreamDestroy(xs); }
    for (hipStream_t ps : h->parked) (void)hipStreamDestroy(ps);
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}


int bn_mppi_set_map(bn_mppi_t *h, int32_t instance, const float *risk, bn_mem_kind where)
{
    if (int rc = check_instance(h, instance, true)) return rc;
    if (!risk) return fail(BN_ERR_INVALID, "risk is null");
    BN_BIND(h);
    if (int rc = settle_point(h)) return rc;
    const size_t bytes = (size_t)h->p.G * h->p.G * 4;
    const hipMemcpyKind kind = where == BN_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const int lo = instance < 0 ? 0 : std::min(instance, h->n_maps - 1);
    const int hi = instance < 0 ? h->n_maps : lo + 1;
    if (int rc = flush_tail(h)) return rc;           // the pending tail rolls X* out on the current map
    BN_HIP(hipStreamSynchronize(h->stream));
    for (int m = lo; m < hi; ++m) BN_HIP(hipMemcpy(h->d_map + (size_t)m * h->p.G * h->p.G, risk, bytes, kind));
    h->map_set = true;
    h->map_epoch += 1;
    return BN_OK;
}

int bn_mppi_set_slip_std(bn_mppi_t *h, int32_t instance, const float *stdv, bn_mem_kind where)
{
    if (int rc = check_instance(h, instance, true)) return rc;
    if (!stdv) return fail(BN_ERR_INVALID, "std is null");
    if (!h->p.slip_on) return fail(BN_ERR_STATE, "handle was created without BN_FLAG_SAMPLED_SLIP");
    BN_BIND(h);
    if (int rc = settle_point(h)) return rc;
    if (int rc = flush_tail(h)) return rc;
    BN_HIP(hipStreamSynchronize(h->stream));
    const size_t bytes = (size_t)h->p.G * h->p.G * 4;
    const hipMemcpyKind kind = where == BN_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const int lo = instance < 0 ? 0 : std::min(instance, h->n_maps - 1), hi = instance < 0 ? h->n_maps : lo + 1;
    for (int m = lo; m < hi; ++m) BN_HIP(hipMemcpy(h->d_slip_std + (size_t)m * h->p.G * h->p.G, stdv, bytes, kind));
    h->slip_std_set = true;
    return BN_OK;
}

int bn_mppi_set_slip_noise(bn_mppi_t *h, const float *zt_device, const float *zc_device, const float *zo_device)
{
    if (!h) return fail(BN_ERR_INVALID, "null handle");
    if (!h->p.slip_on) return fail(BN_ERR_STATE, "handle was created without BN_FLAG_SAMPLED_SLIP");
    if ((zt_device == nullptr) != (zc_device == nullptr) || (zt_device == nullptr) != (zo_device == nullptr))
        return fail(BN_ERR_INVALID, "give all three arrays or none");
    h->p.zt = zt_device; h->p.zc = zc_device; h->p.zo = zo_device;
    return BN_OK;
}

int bn_mppi_set_goal(bn_mppi_t *h, int32_t instance, const float goal_host[2])
{
    if (int rc = check_instance(h, instance, true)) return rc;
    if (!goal_host) return fail(BN_ERR_INVALID, "goal is null");
    BN_BIND(h);
    if (int rc = settle_point(h)) return rc;
    if (int rc = flush_tail(h)) return rc;
    BN_HIP(hipStreamSynchronize(h->stream));
    const int lo = instance < 0 ? 0 : instance, hi = instance < 0 ? h->p.B : instance + 1;
    for (int b = lo; b < hi; ++b) BN_HIP(hipMemcpy(h->d_goal + b * 2, goal_host, 8, hipMemcpyHostToDevice));
    h->goal_set = true;
    return BN_OK;
}

int bn_mppi_set_mean(bn_mppi_t *h, int32_t instance, const float *mean_host)
{
    if (int rc = check_instance(h, instance, true)) return rc;
    BN_BIND(h);
    if (int rc = settle_point(h)) return rc;
    if (int rc = flush_tail(h)) return rc;           // afterwards the mean buffer is authoritative again
    BN_HIP(hipStreamSynchronize(h->stream));
    const size_t n = (size_t)h->p.T * 2;
    const int lo = instance < 0 ? 0 : instance, hi = instance < 0 ? h->p.B : instance + 1;
    for (int b = lo; b < hi; ++b) {
        if (mean_host) BN_HIP(hipMemcpy(h->d_mean + b * n, mean_host, n * 4, hipMemcpyHostToDevice));
        else BN_HIP(hipMemset(h->d_mean + b * n, 0, n * 4));
    }
    return BN_OK;
}

int bn_mppi_sync(bn_mppi_t *h)
{
    if (!h) return fail(BN_ERR_INVALID, "null handle");
    BN_BIND(h);
    hp_cancel(h);
    if (int rc = flush_tail(h)) return rc;
    if (int rc = sync_checked(h)) return rc;            // a bounded device-side wait of an overlapped launch may have expired: see recover_overlap
    return self_check(h);
}

int bn_mppi_order_outputs(bn_mppi_t *h)
{
    if (!h) return fail(BN_ERR_INVALID, "null handle");
    BN_BIND(h);                                         // (that is the call: see hp_order_now)
    return BN_OK;
}

uint64_t bn_mppi_recovery_count(const bn_mppi_t *h) { return h ? h->recoveries : 0; }

int32_t bn_mppi_overlap_mode(const bn_mppi_t *h)
{
    if (!h) return -1;
    const bool capable = (h->lat_kernel || h->role_overlap || h->ticket_overlap) && h->n_streams > 1 && !(h->cfg.flags & (BN_FLAG_PROFILE | BN_FLAG_NO_OVERLAP));
    if (!capable) return 3;
    if (h->overlap_off) return 2;
    return h->tune.chosen ? 1 : 0;
}

int bn_mppi_flush(bn_mppi_t *h)
{
    if (!h) return fail(BN_ERR_INVALID, "null handle");
    BN_BIND(h);
    hp_cancel(h);
    h->hp_gran_valid = false;                          // (the caller may write the mean buffer next: the class's _previous_action_seq setter)
    if (int rc = flush_tail(h)) return rc;
    // no synchronisation here; but an expiry that has ALREADY happened is repaired now rather than at the next synchronising call
    return (h->overlap_used && !h->replaying && __atomic_load_n(h->h_err, __ATOMIC_ACQUIRE)) ? settle_overlap(h, false) : BN_OK;
}

uint64_t bn_mppi_solve_count(const bn_mppi_t *h) { return h ? h->solves - (h->hp_armed ? 1 : 0) : 0; }

const char *bn_last_error(void) { return g_last_error.c_str(); }
int bn_mppi_abi_version(void) { return BN_MPPI_ABI_VERSION; }

}  // extern "C"
