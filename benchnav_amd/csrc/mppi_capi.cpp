// mppi_capi.cpp -- host side of the C ABI declared in include/benchnav_mppi.h: the core.
//
// Owns the device buffers of one planner handle (mppi_handle.h) and enqueues the two kernels of
// a solve (mppi_kernels.hip) on the handle's HIP stream.  No torch types, no CPU
// fallback: creation fails without a gfx950 device.
//
// Here: the error string, the per-device overlap ownership, the journal and the recovery of expired waits,
// create (from the plan of mppi_plan.cpp: register the buffers, allocate, probe) / destroy / setters, and everything a solve executes (solve_impl, bn_mppi_solve_n_async).  The other concerns have a
// file each: mppi_paced.cpp (host-paced loop, forward), mppi_shard.cpp (K-shard exchange), mppi_env.cpp (closed-loop
// environment, DWA), mppi_loops.cpp (A*+DWA and CL-RRT loops), mppi_query.cpp (getters, profiling, lab hooks).
#include "mppi_plan.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cerrno>
#include <sys/stat.h>
#include <fcntl.h>
#include <sys/file.h>
#include <unistd.h>
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
static std::map<int, bn_mppi *> g_overlap_owner;   // device -> the handle whose overlapped batch was enqueued last
// ... and nothing ELSE of this process beside it (round 4).  The rule above kept two overlapped batches apart; a differential sweep
// over pairs of planners (tools/fuzz_features2.py) still saw waits expire: one planner's overlapped batch of latency-kernel
// launches -- one workgroup per CU, sized for a device it has to itself -- with the other planner's ordinary one-stream launches
// in between (12 % of the runs of one pattern, depending on the order the handles' queues were created in).  So a batch
// overlaps only while EVERY other handle on the device is idle (g_handles), and a launch of another handle that arrives while an
// overlapped batch is in flight is ordered behind that batch's end by events (order_behind_foreign_overlap): no host blocking,
// the kernels simply do not share the device with waiting workgroups.
std::map<int, std::vector<bn_mppi *>> g_handles;   // device -> live handles (guarded by g_overlap_mu)
static std::atomic<int> g_overlap_owners{0};              // devices with an owner: the launch path looks at it without the lock
// ... and one PROCESS per device for launches big enough to crowd each other out: two processes with overlapped 64-instance batches
// on one GPU both ran into expired waits within a second.  An advisory lock on a per-device file in /tmp, taken (non-blocking) by
// the first process that overlaps big launches there and held until it exits; a process that does not get it runs those batches
// on one stream and asks again at its next batch.
static std::map<int, int> g_overlap_lock_fd;       // device -> fd holding the lock (-1: not held)

static bool own_device_for_big_overlap(int device)
{
    auto it = g_overlap_lock_fd.find(device);
    if (it != g_overlap_lock_fd.end() && it->second >= 0) return true;
    char bus[64] = "unknown";
    (void)hipDeviceGetPCIBusId(bus, (int)sizeof bus, device);
    for (char *c = bus; *c; ++c)
        if (*c == ':' || *c == '.' || *c == '/') *c = '_';
    const std::string path = std::string("/tmp/benchnav_mppi_overlap_") + bus + ".lock";
    // Read-only open (flock works on it): a file another user created 0644 still opens; no symlink followed in a world-writable
    // directory.  The creator widens the mode past its umask so the next user can do the same.
    const int fd = open(path.c_str(), O_CREAT | O_RDONLY | O_NOFOLLOW | O_CLOEXEC, 0666);
    if (fd < 0) return errno == EROFS || errno == ENOENT;   // no lock file POSSIBLE: behave as a lone process; anything else (EACCES, ELOOP ...): do not overlap
    (void)fchmod(fd, 0666);
    if (flock(fd, LOCK_EX | LOCK_NB) != 0) { close(fd); return false; }
    g_overlap_lock_fd[device] = fd;
    return true;
}

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
        p.ep_index = h->ep_len - 1;
        p.env_z = h->ep_z ? h->ep_z + (size_t)(h->ep_len - 1) * p.B : nullptr;
    }
    p.flag_tail = h->d_flags + kSlots * (size_t)p.B * bn::kFlagStride;        // every tail counts itself in (stream-ordered here: nothing to wait for)
    h->tails += 1;
    if (h->overlap_used) p.err_dev = reinterpret_cast<int *>(h->d_flags + ((kSlots + 1) * (size_t)p.B + 2) * bn::kFlagStride);   // behind overlapped launches: see raise_wait_expired
    if (int rc = guard_foreign_overlap(h)) return rc;
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
    BN_HIP(hipMemset(h->d_flags, 0, ((kSlots + 1) * (size_t)h->p.B + 3) * bn::kFlagStride * sizeof(unsigned long long)));      // counters and the device error word
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
    BN_HIP(hipMemset(h->d_flags, 0, ((kSlots + 1) * (size_t)h->p.B + 3) * bn::kFlagStride * sizeof(unsigned long long)));
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

// Every 64 launches of a batch: how many solves has the device finished (the tails post the first action with the solve's index), and when.
// Two samples that both found the device behind the host give a cadence; anything else says nothing.
static void tune_sample(bn_mppi *h)
{
    if (!h->h_mail || h->in_episode || h->replaying) return;
    bn_mppi::OvSample now;
    now.valid = true;
    now.t = std::chrono::steady_clock::now();
    now.prog = (uint32_t)(__atomic_load_n(h->h_mail, __ATOMIC_ACQUIRE) >> 32);
    now.enq = (uint32_t)h->solves;
    const bn_mppi::OvSample &pr = h->ov_sample;
    if (pr.valid && (int32_t)(pr.enq - now.prog) > 0 && (int32_t)(now.prog - pr.prog) >= 16 && (int32_t)(pr.enq - pr.prog) >= 2) {
        const double us = std::chrono::duration<double, std::micro>(now.t - pr.t).count() / (double)(now.prog - pr.prog);
        tune_record(h, h->run_mode, us);
    }
    h->ov_sample = now;
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
    t.add(&h->d_flags, ((kSlots + 1) * B + 3) * bn::kFlagStride * sizeof(unsigned long long));      // [kSlots][B] + [B] counters, a spare slot, the device error word
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
    unsigned long long *bad = h->d_flags + ((kSlots + 1) * (size_t)p.B + 1) * bn::kFlagStride;      // the spare counter slot, zero
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
    int *probe = reinterpret_cast<int *>(h->d_flags + ((kSlots + 1) * (size_t)h->p.B + 1) * bn::kFlagStride);      // the spare counter slot
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

// A launch of handle h that is not a member of an overlapped batch of its own: if ANOTHER handle's overlapped batch may still be
// in flight on the device, `st` waits for its end (events recorded on that handle's streams).  See g_handles.
static int order_behind_foreign_overlap(bn_mppi *h, hipStream_t st)
{
    std::lock_guard<std::mutex> lock(g_overlap_mu);
    auto it = g_overlap_owner.find(h->cfg.device_id);
    if (it == g_overlap_owner.end() || it->second == h || !it->second) return BN_OK;
    bn_mppi *o = it->second;
    bool busy = false;
    for (int q = 0; q < o->n_streams; ++q) {
        const hipStream_t os = q ? o->xstream[q - 1] : o->stream;
        if (os == st || (q && !os)) continue;                       // the same stream: ordered anyway
        if (hipStreamQuery(os) == hipSuccess) continue;
        busy = true;
        if (!o->ev_guard[q]) continue;
        BN_HIP(hipEventRecord(o->ev_guard[q], os));
        BN_HIP(hipStreamWaitEvent(st, o->ev_guard[q], 0));
    }
    (void)hipGetLastError();
    if (!busy) { g_overlap_owner.erase(it); g_overlap_owners.store((int)g_overlap_owner.size(), std::memory_order_relaxed); }   // its batch is through: nothing to look at until the next one
    return BN_OK;
}


}  // extern "C"

namespace bn {
namespace host {

// Every launch a handle makes on its own stream outside an overlapped batch of its own -- stand-alone tails, re-rolls, environment
// steps and collision checks, not only solves -- goes behind another handle's overlapped batch the same way.
int guard_foreign_overlap(bn_mppi *h)
{
    if (h->last_batch_overlapped || g_overlap_owners.load(std::memory_order_relaxed) == 0) return BN_OK;
    return order_behind_foreign_overlap(h, h->stream);
}

// hp_redo's solve (a lone one-launch solve with its own tail) goes out on a private stream: see hp_redo.
static inline bool lone_self_redo(const bn_mppi *h, bool self_tail, bool overlap)
{
    return h->hp_redo_q >= 0 && self_tail && !overlap && h->lat_kernel && !h->in_episode && !h->tail_pending && !h->replaying && !h->self_off &&
           !(h->cfg.flags & BN_FLAG_NO_PIPELINE);
}

// shard_rollout: the rollouts of a K-sharded solve only (bn_mppi_shard_rollout_async); the tail follows the exchange.
int solve_impl(bn_mppi_t *h, const float *states, bn_mem_kind states_where, const float *eps, bn_noise_kind noise,
               bool shard_rollout, bool overlap, hipStream_t on_stream, int alt_buffers, bool self_tail)
{
    if (!h) return fail(BN_ERR_INVALID, "null handle");
    if (!states) return fail(BN_ERR_INVALID, "states is null");
    if (!h->map_set || !h->goal_set) return fail(BN_ERR_STATE, "set_map and set_goal must precede solve");
    if ((noise == BN_NOISE_PHILOX) != (eps == nullptr))
        return fail(BN_ERR_INVALID, "eps must be NULL exactly when noise == BN_NOISE_PHILOX");
    BN_BIND(h);
    hp_cancel(h);                                      // (a host-paced launch waiting for a state: this solve is not it)
    h->hp_gran_valid = false;
    if (!overlap && g_overlap_owners.load(std::memory_order_relaxed) > 0) {
        if (int rc = order_behind_foreign_overlap(h, on_stream ? on_stream : h->stream)) return rc;
    }

    bn::SolveParams p = h->p;
    const size_t B = p.B, K = p.K, T = p.T;
    h->map_epoch_at_solve = h->map_epoch;
    // Behind an overlapped batch the host has not checked yet (or batches journalled for a re-run): a plain launch's tail must not
    // write the mean from partials of an expired wait either (flush_tail does the same) -- see raise_wait_expired
    if (h->d_flags && (h->overlap_used || !h->journal.empty()))
        p.err_dev = reinterpret_cast<int *>(h->d_flags + ((kSlots + 1) * B + 2) * bn::kFlagStride);
    if (states_where == BN_MEM_DEVICE) {
        p.state = states;
    } else {
        // the pinned block may still feed a previous copy: wait for the stream before reusing it
        if (h->solves) BN_HIP(hipStreamSynchronize(h->stream));
        std::memcpy(h->h_pinned, states, B * 3 * 4);
        BN_HIP(hipMemcpyAsync(h->d_state, h->h_pinned, B * 3 * 4, hipMemcpyHostToDevice, h->stream));
        p.state = h->d_state;
    }
    bn::EpsMode mode = bn::kEpsPhilox;
    switch (noise) {
    case BN_NOISE_PHILOX: break;
    case BN_NOISE_HOST_KT2: {
        const size_t bytes = B * K * T * 2 * 4;
        if (bytes > h->eps_bytes) {
            h->eps_bytes = 0;
            if (int rc = h->bufs.resize(&h->d_eps, bytes, table_fail)) return rc;
            if (int rc = fills_done()) return rc;
            h->eps_bytes = bytes;
        }
        BN_HIP(hipMemcpyAsync(h->d_eps, eps, bytes, hipMemcpyHostToDevice, h->stream));
        p.eps = h->d_eps;
        mode = bn::kEpsKT2;
        break;
    }
    case BN_NOISE_DEVICE_KT2: p.eps = eps; mode = bn::kEpsKT2; break;
    case BN_NOISE_DEVICE_T2K: p.eps = eps; mode = bn::kEpsT2K; break;
    default: return fail(BN_ERR_INVALID, "unknown noise kind %d", (int)noise);
    }

    // Profiling: two-launch mode brackets each kernel with events.  In the pipelined mode a solve is ONE
    // back-to-back launch of ~15 us; an event pair around every launch would add its own ~5 us of
    // dispatch latency, so events are recorded every kProfGroup launches and the mean is taken per group.
    if (shard_rollout) {
        if (int rc = flush_tail(h)) return rc;
        if (h->shard_pending) return fail(BN_ERR_STATE, "the previous sharded solve still waits for bn_mppi_shard_finish_async");
    } else if (h->shard_pending) {
        return fail(BN_ERR_STATE, "a sharded solve waits for bn_mppi_shard_finish_async");
    }
    const bool one_launch = !shard_rollout && (h->pipelined || h->ticket_mode);
    const bool prof_grouped = (h->cfg.flags & BN_FLAG_PROFILE) != 0 && one_launch;
    const bool prof = (h->cfg.flags & BN_FLAG_PROFILE) != 0 && !one_launch;
    hipEvent_t *ev = nullptr;
    if (prof_grouped && h->prof_in_group == 0) {
        if (h->ev_used + 1 > h->ev.size()) {
            hipEvent_t e;
            BN_HIP(hipEventCreate(&e));
            h->ev.push_back(e);
        }
        BN_HIP(hipEventRecord(h->ev[h->ev_used++], h->stream));
    }
    if (prof) {
        if (h->ev_used + 3 > h->ev.size()) {
            for (int i = 0; i < 3; ++i) {
                hipEvent_t e;
                BN_HIP(hipEventCreate(&e));
                h->ev.push_back(e);
            }
        }
        ev = &h->ev[h->ev_used];
        h->ev_used += 3;
        BN_HIP(hipEventRecord(ev[0], h->stream));
    }
    h->last_eps = p.eps;
    h->last_mode = mode;
    const int cur3 = (int)(h->solves % kSlots), prev3 = (int)((h->solves + kSlots - 1) % kSlots);    // per-solve buffers: kSlots slots
    p.solve = h->solves;
    if (h->arm_state_snap) { p.state_snap = h->d_state_snaps + h->snap_slot * (size_t)p.B * 3; h->arm_state_snap = false; }
    p.part = h->d_part[cur3]; p.cost = h->d_cost[cur3]; p.state_copy = h->d_state_copy[cur3];
    p.part_prev = h->d_part[prev3]; p.cost_prev = h->d_cost[prev3]; p.state_prev = h->d_state_copy[prev3];
    if (h->pipelined && !shard_rollout) {
        // one launch: merge + tail of the previous solve ride along with this solve's rollouts
        p.have_prev = h->tail_pending ? 1 : 0;
        p.mean_from_part = h->tail_pending ? 1 : 0;
        p.tail_solve = p.solve - 1;                                   // the tail the aux workgroups write
        if (h->in_episode) {
            // closed loop: from the second step on, the rollout workgroups advance the state themselves
            p.env_on = 1;
            p.closed_loop = (h->ep_len > 0 && h->tail_pending) ? 1 : 0;
            p.ep_index = h->ep_len - 1;                                   // the env step applied / logged by this launch
            p.env_z = (h->ep_z && h->ep_len > 0) ? h->ep_z + (size_t)(h->ep_len - 1) * p.B : nullptr;
            h->ep_len += 1;
        }
        p.wave_kernel = (h->wave_kernel && !h->in_episode) ? 1 : 0;
        if (p.wave_kernel && p.xs == 0 && exp_env("BN_AUX_FIRST")) p.aux_first = 1;      // (experiment builds: VERDICT r5 #3)
        p.lat_kernel = h->lat_kernel ? 1 : 0;
        hipStream_t st = h->stream;
        if (lone_self_redo(h, self_tail, overlap)) st = h->hp_stream[h->hp_redo_q];     // (see hp_redo)
        p.flag_tail = h->d_flags + kSlots * B * bn::kFlagStride;
        if (p.have_prev) {                                             // the aux workgroups write the previous solve's tail
            p.wait_tail = h->tails;                                    // ... after every tail (of the same instance) before it
            h->tails += 1;
        }
        // A synchronous solve on the latency kernel: publishes like a member of a batch (counters, granules) -- for its OWN tail, the second
        // aux workgroup of the same launch; it waits for nobody (no predecessor in flight, no tail pending: the callers see to that).
        const bool lone_self = self_tail && !overlap && h->lat_kernel && !h->in_episode && !p.have_prev && !h->replaying && !h->self_off &&
                               !(h->cfg.flags & BN_FLAG_NO_PIPELINE);
        h->self_tail_launched = false;
        if (lone_self) {
            p.flag_part = h->d_flags;
            p.err = h->d_err; p.err_dev = reinterpret_cast<int *>(h->d_flags + ((kSlots + 1) * B + 2) * bn::kFlagStride);
            p.cur_slot = cur3; p.prev_slot = prev3;
            p.wait_part = h->pub[prev3];
            p.gran = h->d_gran[cur3];                                  // (null above 16 workgroups per instance: the tail waits for the counter)
            p.overlap = 0;
            h->pub[cur3] += (unsigned long long)p.nblk;
            p.self_tail = 1;
            p.wait_part_self = h->pub[cur3];
            p.wait_tail_self = h->tails;
            h->tails += 1;
            p.out_copy_self = h->self_out_copy;
            if (exp_env("BN_NO_EARLY_MAIL")) p.no_early_mail = 1;      // (experiment builds)
            if (h->inline_state && p.B == 1) { p.state_inline = 1; p.sv0 = h->inline_state[0]; p.sv1 = h->inline_state[1]; p.sv2 = h->inline_state[2]; }
            h->self_used = true;
            h->self_tail_launched = true;
            h->prev_published = false;
            h->hp_gran_valid = p.gran != nullptr;
            h->x_idx = 0;
        } else
        if ((h->lat_kernel || h->role_overlap) && overlap) {   // member of an overlapped batch: publishes, and waits if its predecessor published
            p.flag_part = h->d_flags;
            p.err = h->d_err; p.err_dev = reinterpret_cast<int *>(h->d_flags + ((kSlots + 1) * B + 2) * bn::kFlagStride);                                          // pinned host memory, mapped
            if (h->arm_snap) { p.mean_snap = h->d_mean_snap; h->arm_snap = false; }
            p.cur_slot = cur3; p.prev_slot = prev3;
            p.wait_part = h->pub[prev3];
            p.gran = p.lat_kernel ? h->d_gran[cur3] : nullptr;
            if (alt_buffers) {                                         // this solve's trajectories / controls go to one of the extra buffers
                if (h->d_Xalt[alt_buffers - 1]) p.X = h->d_Xalt[alt_buffers - 1];
                if (h->d_Ualt[alt_buffers - 1] && p.U) p.U = h->d_Ualt[alt_buffers - 1];
            }
            p.overlap = (h->prev_published && p.have_prev) ? 1 : 0;
            p.gran_prev = (p.overlap && p.lat_kernel) ? h->d_gran[prev3] : nullptr;
            // every member of the batch runs where the round robin put it -- the first one too (no predecessor to wait for, but if it
            // stayed on the handle's stream while the batch is aligned to END there, solves 0 and 1 would share that stream and solve 2,
            // on the other one, would become eligible before solve 1 is even dispatched: for launches that fill the chip that is the
            // starvation pattern described in bn_mppi_solve_n_async -- 64 instances lost the whole gain of overlapping, 27.5 vs 23.3 us)
            if (on_stream) st = on_stream;
            if (p.overlap) h->overlap_used = true;
            h->pub[cur3] += (unsigned long long)p.nblk;
            h->prev_published = true;
            if (self_tail && p.lat_kernel && !h->in_episode) {         // last solve of a batch: its own tail rides in the same launch
                p.self_tail = 1;
                p.wait_part_self = h->pub[cur3];
                p.wait_tail_self = h->tails;
                h->tails += 1;
            }
        } else {
            h->prev_published = false;
        }
        // more workgroups than the role kernel keeps resident at once (4 per CU x 256 CUs): the aux workgroups run in freed slots
        p.aux_prio = (!p.wave_kernel && (size_t)p.B * (p.nblk + 1) > h->resident_wgs) ? 1 : 0;
        if (!p.wave_kernel && !p.store_u) p.U = nullptr;          // the buffer exists for the throughput kernel only
        if (p.self_tail) BN_HIP(bn::launch_rollout_lat_self(p, mode, st));    // (a kernel of its own: rollout_lat.inc, mode 1)
        else BN_HIP(bn::launch_rollout(p, mode, st));
        if (st != h->stream && lone_self) {                          // hp_redo's solve: what is enqueued on the handle's stream from here on follows it
            BN_HIP(hipEventRecord(h->hp_ev[h->hp_redo_q], st));
            BN_HIP(hipStreamWaitEvent(h->stream, h->hp_ev[h->hp_redo_q], 0));
        }
        if (prof_grouped) h->prof_in_group = (h->prof_in_group + 1) % kProfGroup;
        h->solves += 1;
        h->x_idx = 0;                                  // (batches end on the exposed buffers, bn_mppi_solve_n_async)
        h->tail_pending = !p.self_tail;
        if (p.self_tail) h->prev_published = false;                // the next solve starts from the mean that tail writes, in stream order
        if (lone_self) h->last_batch_overlapped = false;
        return BN_OK;
    }
    if (!(h->ticket_overlap && overlap && !shard_rollout)) h->prev_published = false;
    p.have_prev = 0;
    p.mean_from_part = 0;
    p.tail_solve = p.solve;
    if (p.slip_on && !h->slip_std_set) return fail(BN_ERR_STATE, "bn_mppi_set_slip_std must precede solve in sampled-slip mode");
    if (h->ticket_mode && !shard_rollout) {
        // one launch: the rollouts, the ticket merge of this solve, and the previous solve's tail as aux workgroup
        p.have_prev = h->tail_pending ? 1 : 0;
        p.tail_merged = 1;
        p.tail_solve = p.solve - 1;
        p.ustar_cur = h->d_ustar2[cur3]; p.stats_cur = h->d_stats2[cur3];
        p.ustar_prev = h->d_ustar2[prev3]; p.stats_prev = h->d_stats2[prev3];
        p.ticket = h->d_ticket;
        hipStream_t st = h->stream;
        p.flag_tail = h->d_flags + kSlots * B * bn::kFlagStride;
        if (p.have_prev) { p.wait_tail = h->tails; h->tails += 1; }
        if (h->ticket_overlap && overlap) {
            // member of an overlapped batch (as in the pipelined branch above): the merge of this launch counts itself into its slot
            // (one count per solve), the next launch -- rollouts and tail -- waits for that count instead of for this kernel's end
            p.flag_part = h->d_flags;
            p.err = h->d_err; p.err_dev = reinterpret_cast<int *>(h->d_flags + ((kSlots + 1) * B + 2) * bn::kFlagStride);
            if (h->arm_snap) { p.mean_snap = h->d_mean_snap; h->arm_snap = false; }
            p.cur_slot = cur3; p.prev_slot = prev3;
            p.wait_part = h->pub[prev3];
            if (alt_buffers) {
                if (h->d_Xalt[alt_buffers - 1]) p.X = h->d_Xalt[alt_buffers - 1];
                if (h->d_Ualt[alt_buffers - 1] && p.U) p.U = h->d_Ualt[alt_buffers - 1];
            }
            p.overlap = (h->prev_published && p.have_prev) ? 1 : 0;
            if (on_stream) st = on_stream;
            if (p.overlap) h->overlap_used = true;
            h->pub[cur3] += 1;                                         // one count per instance and solve
            h->prev_published = true;
        }
        if (p.slip_on) BN_HIP(bn::launch_rollout_sampled(p, mode, st));
        else BN_HIP(bn::launch_rollout(p, mode, st));
        if (prof_grouped) h->prof_in_group = (h->prof_in_group + 1) % kProfGroup;
        h->solves += 1;
        h->tail_pending = true;
        return BN_OK;
    }
    // library-enqueued exchange of a K-sharded solve: the shard's rows go straight to their place among the gathered ones (in-place all-gather)
    if (shard_rollout && h->shard_inplace) p.part = h->d_gathered + (size_t)h->shard_rank * p.nblk * (2 + 2 * T);
    if (p.slip_on) {
        BN_HIP(bn::launch_rollout_sampled(p, mode, h->stream));
    } else {
        if (h->slow_path) p.wave_kernel = 1;                 // no control tile in LDS, any horizon; REF arithmetic when p.ref_order
        else if (!p.store_u) p.U = nullptr;                  // (the buffer may exist for the throughput kernel only)
        BN_HIP(bn::launch_rollout(p, mode, h->stream));
    }
    if (prof) BN_HIP(hipEventRecord(ev[1], h->stream));
    if (shard_rollout) {
        if (prof) BN_HIP(hipEventRecord(ev[2], h->stream));
        h->solves += 1;
        h->tail_pending = false;
        h->shard_pending = true;
        return BN_OK;
    }
    p.state = p.state_copy;
    BN_HIP(bn::launch_finish(p, h->stream));
    if (prof) BN_HIP(hipEventRecord(ev[2], h->stream));
    h->solves += 1;
    h->tail_pending = false;
    return BN_OK;
}

}  // namespace host
}  // namespace bn

extern "C" {

int bn_mppi_solve_async(bn_mppi_t *h, const float *states, bn_mem_kind states_where, const float *eps,
                        bn_noise_kind noise)
{
    if (h && !h->replaying && !h->journal.empty()) {
        // a single solve behind overlapped batches whose error word has not been checked yet: journalled as a batch of one
        h->last_batch_overlapped = false;
        journal_arm_states(h);
        journal_push(h, bn_mppi::BatchRec{1, states, eps, noise, 1, 0, false, nullptr}, states_where == BN_MEM_DEVICE && noise != BN_NOISE_HOST_KT2);
    }
    return solve_impl(h, states, states_where, eps, noise, false);
}

int bn_mppi_solve_n_async(bn_mppi_t *h, int32_t n, const float *states, bn_mem_kind states_where, const float *eps,
                          bn_noise_kind noise, int32_t eps_ring, int64_t eps_stride)
{
    if (n < 0) return fail(BN_ERR_INVALID, "n must be >= 0");
    if (eps && (eps_ring < 1 || eps_stride < 0)) return fail(BN_ERR_INVALID, "eps_ring must be >= 1 and eps_stride >= 0");
    if (!h) return fail(BN_ERR_INVALID, "null handle");
    // Overlapped launches.  Solve i+1 needs only the softmin partials of solve i, yet in one stream it also waits for solve i's
    // kernel to drain and for the dispatch of its own (~2.4 us of a 13 us step).  With the latency kernel consecutive solves
    // alternate between the handle's stream and a second one: solve i+1 is dispatched while solve i runs, stages its window and
    // draws its first noise, and then waits on a device counter for solve i's partials (published as device-scope stores by
    // the workgroups themselves).  At most two launches are in flight (each stream serialises its own); per-solve buffers
    // rotate over three slots so that what a launch overwrites was last read by a launch that has completed on its stream;
    // the tails (aux workgroups) are ordered by a second counter.  Results are bit-identical to the one-stream chain.
    // Device-side episodes overlap the same way (role kernel): the successor reads the state its predecessor advanced with
    // device-scope loads after its wait (64 instances: 29.6 -> 24.8 us per control step).
    const bool overlap = (h->lat_kernel || h->role_overlap || h->ticket_overlap) && h->n_streams > 1 && (h->d_Xalt[0] || h->p.lean) && n >= 3 && states_where == BN_MEM_DEVICE &&
                         noise != BN_NOISE_HOST_KT2 && !(h->cfg.flags & (BN_FLAG_PROFILE | BN_FLAG_NO_OVERLAP)) && !h->shard_pending && !h->overlap_off;
    // which mode this batch runs in: the handle's choice, or -- for its first 192 launches, once -- the other one, for a look (tune_record)
    int mode = overlap ? h->tune.chosen : 1;
    if (overlap && h->tune.explore && n >= 128 && !h->in_episode && !h->replaying) {
        const int32_t ring = eps ? eps_ring : 1;
        const int32_t prefix = ((192 + ring - 1) / ring) * ring;       // (a whole number of turns of the caller's noise ring: the rest starts at block 0 again)
        if (n > prefix + 2) {
            if (int rc = bn_mppi_solve_n_async(h, prefix, states, states_where, eps, noise, eps_ring, eps_stride)) return rc;
            h->tune.explore = 0;                                        // (looked, whether or not the windows were conclusive)
            return bn_mppi_solve_n_async(h, n - prefix, states, states_where, eps, noise, eps_ring, eps_stride);
        }
        mode = 1 - h->tune.chosen;
    }
    if (mode != h->run_mode) h->ov_sample.valid = false;
    h->run_mode = mode;
    bool mine = overlap && mode == 0;
    if (mine) {                                         // see g_overlap_owner
        BN_BIND(h);
        std::lock_guard<std::mutex> lock(g_overlap_mu);
        bn_mppi *&owner = g_overlap_owner[h->cfg.device_id];
        if (owner && owner != h) {                      // is the owner's latest overlapped batch still in flight?
            bool busy = hipStreamQuery(owner->stream) != hipSuccess;
            for (int q = 0; !busy && q + 1 < owner->n_streams; ++q) busy = hipStreamQuery(owner->xstream[q]) != hipSuccess;
            (void)hipGetLastError();
            if (busy) mine = false;
        }
        for (bn_mppi *o : g_handles[h->cfg.device_id]) {   // ... and is every other handle idle?  (see g_handles)
            if (!mine) break;
            if (o == h) continue;
            for (int q = 0; mine && q < kMaxStreams; ++q) {            // (incl. the second private stream of a host-paced handle)
                const hipStream_t os = q ? o->xstream[q - 1] : o->stream;
                if ((q && !os) || os == h->stream) continue;
                if (hipStreamQuery(os) != hipSuccess) mine = false;
            }
        }
        (void)hipGetLastError();
        const size_t slots_ = h->wave_kernel ? 24 * (size_t)std::max(h->n_cus, 1) : (h->lat_kernel ? (size_t)std::max(h->n_cus, 1) : h->resident_wgs);
        if (mine && 2 * (size_t)h->p.B * (h->p.nblk + 1) > slots_ && !own_device_for_big_overlap(h->cfg.device_id)) mine = false;
        // A launch that needs well over one residency round by itself is never fully placed while it runs: its successor's waiting
        // workgroups compete with its OWN remaining ones for every slot that frees up, whatever the host orders.  Up to a quarter over
        // (64 instances of K = 1024: 1088 workgroups on 1024 slots; 70: 1190) the remainder is placed when the first round drains and
        // nothing has ever expired (tens of thousands of launches, fresh processes included); at one and a half rounds (3 instances of
        // K = 8192 at one workgroup per CU: 387 on 256) the first batch of a fresh process expired every time (round 4,
        // tests/differential.py `ops` seed 2681).  Such batches run on one stream.
        if (mine && 4 * (size_t)h->p.B * (h->p.nblk + 1) > 5 * slots_) mine = false;
        if (mine) owner = h;
        else if (!owner) g_overlap_owner.erase(h->cfg.device_id);      // (operator[] above created an empty entry)
        g_overlap_owners.store((int)g_overlap_owner.size(), std::memory_order_relaxed);
    }
    const bn_mppi::BatchRec rec{n, states, eps, noise, eps_ring, eps_stride, false, nullptr};
    const bool replayable = states_where == BN_MEM_DEVICE && noise != BN_NOISE_HOST_KT2;
    if (replayable && !h->in_episode) journal_arm_states(h);
    if (!mine) {
        h->last_batch_overlapped = false;
        for (int32_t i = 0; i < n; ++i) {
            const float *e = eps ? eps + (size_t)(i % eps_ring) * (size_t)eps_stride : nullptr;
            if (int rc = solve_impl(h, states, states_where, e, noise, false)) return rc;
            if (overlap && (i & 63) == 63) tune_sample(h);
        }
        if (!h->in_episode) journal_push(h, rec, replayable);   // behind an overlapped batch not yet checked: lost with it, re-run with it
        return BN_OK;
    }
    BN_BIND(h);
    h->last_batch_overlapped = true;
    if (!h->replaying && h->journal.empty() && !h->journal_lost) {   // first batch since the error word was last seen clean
        h->journal_solves0 = h->solves;
        h->arm_snap = true;
    }
    const int S = h->n_streams;
    // The scheme relies on a launch having been dispatched before its successor becomes eligible: waiting workgroups hold their
    // slots, and the hardware does not share freed slots fairly between two queues (seen with two 70-instance launches made
    // eligible at the same instant: the successor's waiting workgroups took every slot, the predecessor's never got one, the
    // waits expired).  Inside a batch that holds by construction -- launch i+1 becomes eligible when launch i-1 completes, a whole
    // kernel after launch i did.  At the START it holds when the stream is idle (solve 1 is enqueued microseconds after solve 0
    // went out); if earlier work is still pending, solves 0 and 1 would become eligible together, so launches big enough to
    // crowd each other out wait for the stream first.
    const size_t slots = h->wave_kernel ? 24 * (size_t)std::max(h->n_cus, 1) : (h->lat_kernel ? (size_t)std::max(h->n_cus, 1) : h->resident_wgs);
    bool idle = hipStreamQuery(h->stream) == hipSuccess;
    (void)hipGetLastError();
    if (!idle && 2 * (size_t)h->p.B * (h->p.nblk + 1) > slots) {
        BN_HIP(hipStreamSynchronize(h->stream));
        idle = true;
    }
    if (!idle) {                                                    // fork: the extra streams start behind everything enqueued so far
        BN_HIP(hipEventRecord(h->ev_fork, h->stream));              // (nothing is: no event packet in front of the first launches)
        for (int q = 0; q + 1 < S; ++q) BN_HIP(hipStreamWaitEvent(h->xstream[q], h->ev_fork, 0));
    }
    // The last launch of a long batch carries its own tail as a second aux workgroup (SolveParams::self_tail; the one-launch kernel,
    // rollout_lat.inc mode 1) instead of a tail kernel behind it: since round 6 that workgroup stages its window while the rollouts run
    // and polls the granules of their rows -- 3 us off a 20-solve region (tools/region_ab.py: 215.2 -> 212.2 us; the counter-waiting
    // tail of rounds 2-5 had measured 5 us WORSE than the kernel behind).  BN_NO_SELF_TAIL (experiment builds) turns it off.
    const bool exp_self_tail = exp_env("BN_NO_SELF_TAIL") == nullptr;      // (read per batch: tools/region_ab.py toggles it inside one process)
    static const bool exp_align = exp_env("BN_NO_ALIGN") == nullptr;
    if (!exp_align) idle = false;                                   // (only the stream assignment below looks at it from here on)
    // Launches big enough to crowd each other out start on the handle's OWN stream, whatever that costs at the batch's end.  Aligning
    // the round robin to end there puts solve 0 of an even batch on the internal stream -- a queue that has been idle since the last
    // batch and wakes up later than the handle's, which has just carried the caller's work: solve 1 was then dispatched BEFORE solve 0,
    // its waiting workgroups took the slots solve 0 needed, and the bounded waits expired (round 4, tools/_seq tests: 3-7 of 18 fresh
    // 64-instance handles with even batch lengths, none with odd ones; it is what made test_big_batches_... fail one run in eight).
    const bool crowd = 2 * (size_t)h->p.B * (h->p.nblk + 1) > slots;
    if (crowd && !exp_env("BN_ALIGN_BIG")) idle = false;      // (BN_ALIGN_BIG: tools/recovery_stress.py brings the race back)
    int rc = BN_OK;
    int stamp = 0;
    for (int32_t i = 0; i < n && rc == BN_OK; ++i) {
        const float *e = eps ? eps + (size_t)(i % eps_ring) * (size_t)eps_stride : nullptr;
        // Stream (and trajectory buffer) of solve i: round robin, except that the LAST solve always runs on the handle's own stream
        // -- whatever follows it there (the batch's tail kernel, a getter) is then ordered by the queue itself instead of by a
        // cross-queue event that has only just fired (measured: 18 us between the last rollout kernel and the tail).  With an
        // even n the last two solves share the stream, which costs one overlap.  (Not the first two: the solve on the other
        // stream would then become eligible before its predecessor is even dispatched -- see the note on eligibility above.)
        // On an idle stream nothing ties the first solve to the handle's stream, so the round robin is simply aligned to END there.
        const int q = idle ? (n - 1 - i) % S : (i == n - 1 ? 0 : i % S);
        // A long batch ends with its own tail (see below): on the latency kernel it rides in the last launch as a second aux workgroup.
        const bool own_tail = i == n - 1 && n >= kEagerTailMinBatch && exp_self_tail;
        // A launch that exceeds one residency round (`over` below; up to 1.25 rounds overlap at all, see `mine`): a launch whose workgroups
        // wait for partials holds slots, and the dispatcher does not share freed slots fairly between two queues -- a successor that
        // becomes eligible while its predecessor still has workgroups to place can take every slot and starve it until the bounded waits
        // expire.  In the steady state that cannot happen: launch i+1 becomes eligible when launch i-1 completes, a whole kernel after
        // launch i did.  The START of a batch is different -- the second launch goes to a queue that has been idle and wakes up late
        // (8 us and more in the kernel traces): it could be dispatched before the first (the inversion the stream assignment above made
        // rare), or so late that the THIRD launch, eligible when the first completes, finds it half placed (round 4,
        // tools/fuzz_features.py: every expiry on a 70-instance planner was the third launch of a batch waiting for workgroups of the
        // second that never got a slot: one handle in 20 to 400, box by box, each repaired by a re-run).  So the first three launches
        // are handed over one by one: a one-thread marker kernel in front of a launch stamps pinned host memory when its queue has
        // reached it, and the host enqueues the next launch only then -- the other queue is woken by a marker of its own right away.
        // A few microseconds of host time under a first launch of 20 us and more, once per batch.  (The stamps cannot come from the
        // rollout kernels themselves: two more live scalars in their prologues put the role kernel on the register allocator's
        // emergency slot, tests/test_build_artifacts.py.)
        const hipStream_t qs = q ? h->xstream[q - 1] : h->stream;
        auto seen = [&](int word, hipStream_t wait_out) -> int {
            const auto t0 = std::chrono::steady_clock::now();
            while (__atomic_load_n(&h->h_err[word], __ATOMIC_ACQUIRE) != stamp) {
                if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) {      // something else holds the GPU: wait the launch out
                    BN_HIP(hipStreamSynchronize(wait_out));
                    break;
                }
            }
            return BN_OK;
        };
        // Only launches that exceed one residency round by THEMSELVES can be starved for good (a waiting launch of at most one round
        // leaves its predecessor's running workgroups to finish and free what the rest of it needs): two launches that merely do not
        // fit side by side -- 256 instances on the one-wave kernel, K = 16384 -- skip the hand-over.
        const bool over = (size_t)h->p.B * (h->p.nblk + 1) > slots;
        if (over && !h->replaying && n >= 3 && i < 3) {
            if (i == 0) {
                stamp = (int)(h->solves & 0x3fffffff) + 1;
                for (int w = 4; w < 8; ++w) __atomic_store_n(&h->h_err[w], 0, __ATOMIC_RELEASE);
                if (S > 1) BN_HIP(bn::launch_stamp(h->d_err + 5, stamp, h->xstream[0]));      // wakes the other queue
                BN_HIP(bn::launch_stamp(h->d_err + 4, stamp, qs));
            } else if (i == 1) {
                if (int r = seen(4, h->stream)) return r;                                          // the first launch is next in a queue that is being processed
                if (S > 1) { if (int r = seen(5, h->xstream[0])) return r; }
                BN_HIP(bn::launch_stamp(h->d_err + 6, stamp, qs));
            } else {
                if (int r = seen(6, h->xstream[0])) return r;                                      // ... and so is the second
            }
        }
        rc = solve_impl(h, states, states_where, e, noise, false, true, qs, q, own_tail);
        if ((i & 63) == 63) tune_sample(h);
    }
    // A long batch ends with its own tail, enqueued right behind the last solve and BEFORE the join: a tail kernel that comes later
    // (flush, sync, a getter) would sit behind the join's barrier packet, ~10 us of queue processing after the last rollout kernel.
    // Short batches keep the tail pending: chained short batches carry it in their next launch for free.
    if (rc == BN_OK && n >= kEagerTailMinBatch && !h->in_episode) rc = flush_tail(h);
    static const bool exp_join = exp_env("BN_JOIN") != nullptr;   // experiments (tools/region_overhead.py)
    for (int q = 0; exp_join && q + 1 < S; ++q) {                   // join: the handle's stream continues behind all of them
        hipError_t e1 = hipEventRecord(h->ev_join[q], h->xstream[q]);
        hipError_t e2 = hipStreamWaitEvent(h->stream, h->ev_join[q], 0);
        if (rc == BN_OK && (e1 != hipSuccess || e2 != hipSuccess)) rc = fail(BN_ERR_HIP, "joining the overlapped launches failed");
    }
    if (rc == BN_OK && !h->in_episode) journal_push(h, rec, replayable);
    return rc;
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

int bn_mppi_solve(bn_mppi_t *h, const float *states, bn_mem_kind states_where, const float *eps,
                  bn_noise_kind noise, float *ustar_host, float *xstar_host)
{
    if (!h) return fail(BN_ERR_INVALID, "null handle");
    BN_BIND(h);
    if (int rc = settle_point(h)) return rc;
    if (h->lat_kernel && h->tail_pending && !h->self_off) { if (int rc = flush_tail(h)) return rc; }      // (as in forward_impl)
    if (int rc = solve_impl(h, states, states_where, eps, noise, false, false, nullptr, 0, true)) return rc;   // own tail in the launch where that exists
    if (int rc = flush_tail(h)) return rc;
    const size_t B = h->p.B, T = h->p.T;
    if (ustar_host) BN_HIP(hipMemcpyAsync(ustar_host, h->d_ustar, B * T * 2 * 4, hipMemcpyDeviceToHost, h->stream));
    if (xstar_host)
        BN_HIP(hipMemcpyAsync(xstar_host, h->d_xstar, B * (T + 1) * 3 * 4, hipMemcpyDeviceToHost, h->stream));
    BN_HIP(hipStreamSynchronize(h->stream));
    return self_check(h);
}

uint64_t bn_mppi_solve_count(const bn_mppi_t *h) { return h ? h->solves - (h->hp_armed ? 1 : 0) : 0; }

const char *bn_last_error(void) { return g_last_error.c_str(); }
int bn_mppi_abi_version(void) { return BN_MPPI_ABI_VERSION; }

}  // extern "C"
