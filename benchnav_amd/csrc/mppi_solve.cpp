// mppi_solve.cpp -- the solve path of the C ABI: everything that runs per control step.  solve_impl in steps -- checks, staging of
// state and noise, profiling events, the launch decision of one of three paths (pipelined, ticket, two launches / shard rollouts), its
// application (mppi_launch.h), the bookkeeping behind the launch -- and bn_mppi_solve_async, bn_mppi_solve_n_async (overlapped
// batches: eligibility, the tuner's look at the other mode, the claim of the device, the stream of every solve, the hand-over of the
// first launches, the batch's tail and journal record) and bn_mppi_solve.  A launch of a handle that is not a member of an overlapped
// batch of its own goes behind another handle's overlapped batch here (guard_foreign_overlap).
#include "mppi_launch.h"

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <cstring>
#include <fcntl.h>
#include <map>
#include <mutex>
#include <string>
#include <sys/file.h>
#include <sys/stat.h>
#include <unistd.h>

namespace bn {
namespace host {

// ... and one PROCESS per device for launches big enough to crowd each other out (see g_overlap_owner, mppi_capi.cpp): two processes
// with overlapped 64-instance batches
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

// Every launch a handle makes on its own stream outside an overlapped batch of its own -- stand-alone tails, re-rolls, environment
// steps and collision checks, not only solves -- goes behind another handle's overlapped batch the same way.
int guard_foreign_overlap(bn_mppi *h)
{
    if (h->last_batch_overlapped || g_overlap_owners.load(std::memory_order_relaxed) == 0) return BN_OK;
    return order_behind_foreign_overlap(h, h->stream);
}

namespace {

// What the caller of solve_impl asked for, and the noise layout its staging settled.
struct SolveCall { bool shard_rollout, overlap; int q; bool self_tail; bn::EpsMode mode; };
// The profiling events of this solve: `grouped` = one event per kProfGroup launches, `ev` = the three events of a two-launch solve.
struct Prof { bool grouped = false; hipEvent_t *ev = nullptr; };

int check_solve_args(const bn_mppi *h, const float *states, const float *eps, bn_noise_kind noise)
{
    if (!h) return fail(BN_ERR_INVALID, "null handle");
    if (!states) return fail(BN_ERR_INVALID, "states is null");
    if (!h->map_set || !h->goal_set) return fail(BN_ERR_STATE, "set_map and set_goal must precede solve");
    if ((noise == BN_NOISE_PHILOX) != (eps == nullptr))
        return fail(BN_ERR_INVALID, "eps must be NULL exactly when noise == BN_NOISE_PHILOX");
    return BN_OK;
}

int stage_state(bn_mppi *h, bn::SolveParams &p, const float *states, bn_mem_kind states_where)
{
    const size_t B = p.B;
    if (states_where == BN_MEM_DEVICE) {
        p.state = states;
    } else {
        // the pinned block may still feed a previous copy: wait for the stream before reusing it
        if (h->solves) BN_HIP(hipStreamSynchronize(h->stream));
        std::memcpy(h->h_pinned, states, B * 3 * 4);
        BN_HIP(hipMemcpyAsync(h->d_state, h->h_pinned, B * 3 * 4, hipMemcpyHostToDevice, h->stream));
        p.state = h->d_state;
    }
    return BN_OK;
}

int stage_noise(bn_mppi *h, bn::SolveParams &p, const float *eps, bn_noise_kind noise, bn::EpsMode *mode)
{
    const size_t B = p.B, K = p.K, T = p.T;
    *mode = bn::kEpsPhilox;
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
        *mode = bn::kEpsKT2;
        break;
    }
    case BN_NOISE_DEVICE_KT2: p.eps = eps; *mode = bn::kEpsKT2; break;
    case BN_NOISE_DEVICE_T2K: p.eps = eps; *mode = bn::kEpsT2K; break;
    default: return fail(BN_ERR_INVALID, "unknown noise kind %d", (int)noise);
    }
    return BN_OK;
}

// The rollouts of a K-sharded solve start from a written tail; nothing else runs between them and bn_mppi_shard_finish_async.
int check_shard_order(bn_mppi *h, bool shard_rollout)
{
    if (shard_rollout) {
        if (int rc = flush_tail(h)) return rc;
        if (h->shard_pending) return fail(BN_ERR_STATE, "the previous sharded solve still waits for bn_mppi_shard_finish_async");
    } else if (h->shard_pending) {
        return fail(BN_ERR_STATE, "a sharded solve waits for bn_mppi_shard_finish_async");
    }
    return BN_OK;
}

// Profiling: two-launch mode brackets each kernel with events.  In the pipelined mode a solve is ONE
// back-to-back launch of ~15 us; an event pair around every launch would add its own ~5 us of
// dispatch latency, so events are recorded every kProfGroup launches and the mean is taken per group.
int prof_begin(bn_mppi *h, bool one_launch, Prof *prof)
{
    if (!(h->cfg.flags & BN_FLAG_PROFILE)) return BN_OK;
    prof->grouped = one_launch;
    if (one_launch) {
        if (h->prof_in_group != 0) return BN_OK;
        if (h->ev_used + 1 > h->ev.size()) {
            hipEvent_t e;
            BN_HIP(hipEventCreate(&e));
            h->ev.push_back(e);
        }
        BN_HIP(hipEventRecord(h->ev[h->ev_used++], h->stream));
        return BN_OK;
    }
    if (h->ev_used + 3 > h->ev.size()) {
        for (int i = 0; i < 3; ++i) {
            hipEvent_t e;
            BN_HIP(hipEventCreate(&e));
            h->ev.push_back(e);
        }
    }
    prof->ev = &h->ev[h->ev_used];
    h->ev_used += 3;
    BN_HIP(hipEventRecord(prof->ev[0], h->stream));
    return BN_OK;
}

inline void prof_count_launch(bn_mppi *h, const Prof &prof)
{
    if (prof.grouped) h->prof_in_group = (h->prof_in_group + 1) % kProfGroup;
}

inline int launch_family(const bn_mppi_launch_record &r) { return r.entry != kRollout ? 0 : (r.wave_kernel ? 1 : (r.lat_kernel ? 2 : 0)); }

// ---- decide: what the launch of each path will be.  No HIP call, the handle is only read. ---------------------------------------

// one launch: merge + tail of the previous solve ride along with this solve's rollouts
LaunchDecision decide_pipelined(const bn_mppi *h, const SolveCall &c, LaunchDecision d)
{
    bn_mppi_launch_record &r = d.r;
    const bn::SolveParams &p = h->p;
    r.have_prev = r.mean_from_part = h->tail_pending ? 1 : 0;
    r.tail_solve = r.solve - 1;                                        // the tail the aux workgroups write
    if (h->in_episode) {
        // closed loop: from the second step on, the rollout workgroups advance the state themselves
        r.env_on = 1;
        r.closed_loop = (h->ep_log.len > 0 && h->tail_pending) ? 1 : 0;
        r.ep_index = h->ep_log.len - 1;                                    // the env step applied / logged by this launch
        r.env_z = (h->ep_z && h->ep_log.len > 0) ? 1 : 0;
    }
    r.wave_kernel = (h->wave_kernel && !h->in_episode) ? 1 : 0;
    r.lat_kernel = h->lat_kernel ? 1 : 0;
    r.flag_tail = 1;
    if (r.have_prev) {                                                 // the aux workgroups write the previous solve's tail
        r.wait_tail = h->tails;                                        // ... after every tail (of the same instance) before it
        d.tails = 1;
    }
    if (lone_self_solve(h, c.self_tail, c.overlap)) {
        d.lone_self = true;
        r.flag_part = r.err = r.err_dev = 1;
        r.cur_slot = d.cur; r.prev_slot = d.prev;
        r.wait_part = h->pub[d.prev];
        r.gran = h->d_gran[d.cur] ? 1 : 0;                             // (none above 16 workgroups per instance: the tail waits for the counter)
        d.publish = (unsigned long long)p.nblk;
        carry_own_tail(h, d);
        r.out_copy_self = h->self_out_copy ? 1 : 0;
        r.state_inline = (h->inline_state && p.B == 1) ? 1 : 0;
        if (h->hp_redo_q >= 0) r.stream = 1 + h->hp_redo_q;            // hp_redo's solve goes out on a private stream: see hp_redo
    } else if ((h->lat_kernel || h->role_overlap) && c.overlap) {      // member of an overlapped batch: publishes, and waits if its predecessor published
        // every member of the batch runs where the round robin put it -- the first one too (no predecessor to wait for, but if it
        // stayed on the handle's stream while the batch is aligned to END there, solves 0 and 1 would share that stream and solve 2,
        // on the other one, would become eligible before solve 1 is even dispatched: for launches that fill the chip that is the
        // starvation pattern described in bn_mppi_solve_n_async -- 64 instances lost the whole gain of overlapping, 27.5 vs 23.3 us)
        join_batch(h, d, c.q, (unsigned long long)p.nblk, r.lat_kernel != 0);
        if (c.self_tail && r.lat_kernel && !h->in_episode) carry_own_tail(h, d);      // last solve of a batch: its own tail rides in the same launch
    }
    // more workgroups than the role kernel keeps resident at once (4 per CU x 256 CUs): the aux workgroups run in freed slots
    r.aux_prio = (!r.wave_kernel && (size_t)p.B * (p.nblk + 1) > h->resident_wgs) ? 1 : 0;
    if (!r.wave_kernel && !p.store_u) r.u_buf = -1;                    // the buffer exists for the throughput kernel only
    r.entry = r.self_tail ? kRolloutLatSelf : kRollout;                // (a kernel of its own: rollout_lat.inc, mode 1)
    r.family = launch_family(r);
    return d;
}

// one launch: the rollouts, the ticket merge of this solve, and the previous solve's tail as aux workgroup
LaunchDecision decide_ticket(const bn_mppi *h, const SolveCall &c, LaunchDecision d)
{
    bn_mppi_launch_record &r = d.r;
    r.have_prev = h->tail_pending ? 1 : 0;
    r.tail_merged = 1;
    r.tail_solve = r.solve - 1;
    r.flag_tail = 1;
    if (r.have_prev) { r.wait_tail = h->tails; d.tails = 1; }
    // member of an overlapped batch (as in the pipelined path): the merge of this launch counts itself into its slot (one count per
    // instance and solve), the next launch -- rollouts and tail -- waits for that count instead of for this kernel's end
    if (h->ticket_overlap && c.overlap) join_batch(h, d, c.q, 1, false);
    r.entry = h->p.slip_on ? kRolloutSampled : kRollout;
    r.family = launch_family(r);
    return d;
}

// two launches: the rollouts here, the tail behind them (or, for a K-sharded solve, behind the exchange)
LaunchDecision decide_two_launches(const bn_mppi *h, const SolveCall &c, LaunchDecision d)
{
    bn_mppi_launch_record &r = d.r;
    r.tail_solve = r.solve;
    // library-enqueued exchange of a K-sharded solve: the shard's rows go straight to their place among the gathered ones (in-place all-gather)
    r.part_gathered = (c.shard_rollout && h->shard_inplace) ? 1 : 0;
    if (h->p.slip_on) {
        r.entry = kRolloutSampled;
    } else {
        r.entry = kRollout;
        if (h->slow_path) r.wave_kernel = 1;                 // no control tile in LDS, any horizon; REF arithmetic when p.ref_order
        else if (!h->p.store_u) r.u_buf = -1;                // (the buffer may exist for the throughput kernel only)
    }
    r.family = launch_family(r);
    return d;
}

// ---- one function per path: decide, apply, launch, and the bookkeeping behind the launch ------------------------------------------

int solve_pipelined(bn_mppi *h, bn::SolveParams &p, const SolveCall &c, const LaunchDecision &d0, const Prof &prof)
{
    const LaunchDecision d = decide_pipelined(h, c, d0);
    if (h->in_episode) h->ep_log.len += 1;
    h->self_tail_launched = d.lone_self;
    if (d.lone_self) {
        h->self_used = true;
        h->hp_gran_valid = d.r.gran != 0;
        h->x_idx = 0;
    }
    h->prev_published = d.member;
    apply_decision(h, p, d);
    if (p.wave_kernel && p.xs == 0 && exp_env("BN_AUX_FIRST")) p.aux_first = 1;      // (experiment builds: VERDICT r5 #3)
    if (d.lone_self && exp_env("BN_NO_EARLY_MAIL")) p.no_early_mail = 1;               // (experiment builds)
    const hipStream_t st = launch_stream(h, d.r.stream);
    if (d.r.entry == kRolloutLatSelf) BN_HIP(bn::launch_rollout_lat_self(p, c.mode, st));
    else BN_HIP(bn::launch_rollout(p, c.mode, st));
    if (st != h->stream && d.lone_self) {                          // hp_redo's solve: what is enqueued on the handle's stream from here on follows it
        BN_HIP(hipEventRecord(h->hp_ev[h->hp_redo_q], st));
        BN_HIP(hipStreamWaitEvent(h->stream, h->hp_ev[h->hp_redo_q], 0));
    }
    prof_count_launch(h, prof);
    h->solves += 1;
    h->x_idx = 0;                                  // (batches end on the exposed buffers, bn_mppi_solve_n_async)
    h->tail_pending = !d.r.self_tail;
    if (d.r.self_tail) h->prev_published = false;              // the next solve starts from the mean that tail writes, in stream order
    if (d.lone_self) h->last_batch_overlapped = false;
    return BN_OK;
}

int solve_ticket(bn_mppi *h, bn::SolveParams &p, const SolveCall &c, const LaunchDecision &d0, const Prof &prof)
{
    const LaunchDecision d = decide_ticket(h, c, d0);
    p.ustar_cur = h->d_ustar2[d.cur]; p.stats_cur = h->d_stats2[d.cur];
    p.ustar_prev = h->d_ustar2[d.prev]; p.stats_prev = h->d_stats2[d.prev];
    p.ticket = h->d_ticket;
    if (d.member) h->prev_published = true;
    apply_decision(h, p, d);
    const hipStream_t st = launch_stream(h, d.r.stream);
    if (d.r.entry == kRolloutSampled) BN_HIP(bn::launch_rollout_sampled(p, c.mode, st));
    else BN_HIP(bn::launch_rollout(p, c.mode, st));
    prof_count_launch(h, prof);
    h->solves += 1;
    h->tail_pending = true;
    return BN_OK;
}

int solve_two_launches(bn_mppi *h, bn::SolveParams &p, const SolveCall &c, const LaunchDecision &d0, const Prof &prof)
{
    LaunchDecision d = decide_two_launches(h, c, d0);
    apply_decision(h, p, d);
    if (d.r.part_gathered) p.part = h->d_gathered + (size_t)h->shard_rank * p.nblk * (2 + 2 * (size_t)p.T);
    if (d.r.entry == kRolloutSampled) BN_HIP(bn::launch_rollout_sampled(p, c.mode, h->stream));
    else BN_HIP(bn::launch_rollout(p, c.mode, h->stream));
    if (prof.ev) BN_HIP(hipEventRecord(prof.ev[1], h->stream));
    if (c.shard_rollout) {
        if (prof.ev) BN_HIP(hipEventRecord(prof.ev[2], h->stream));
        h->solves += 1;
        h->tail_pending = false;
        h->shard_pending = true;
        return BN_OK;
    }
    p.state = p.state_copy;
    d.r.entry = kFinish; d.r.family = 0;
    log_launch(h, d.r);
    BN_HIP(bn::launch_finish(p, h->stream));
    if (prof.ev) BN_HIP(hipEventRecord(prof.ev[2], h->stream));
    h->solves += 1;
    h->tail_pending = false;
    return BN_OK;
}

}  // namespace

// shard_rollout: the rollouts of a K-sharded solve only (bn_mppi_shard_rollout_async); the tail follows the exchange.
int solve_impl(bn_mppi_t *h, const float *states, bn_mem_kind states_where, const float *eps, bn_noise_kind noise,
               bool shard_rollout, bool overlap, int q, bool self_tail)
{
    if (int rc = check_solve_args(h, states, eps, noise)) return rc;
    BN_BIND(h);
    hp_cancel(h);                                      // (a host-paced launch waiting for a state: this solve is not it)
    h->hp_gran_valid = false;
    if (!overlap && g_overlap_owners.load(std::memory_order_relaxed) > 0) {
        if (int rc = order_behind_foreign_overlap(h, h->stream)) return rc;
    }

    bn::SolveParams p = h->p;
    SolveCall c{shard_rollout, overlap, q, self_tail, bn::kEpsPhilox};
    LaunchDecision d;
    h->map_epoch_at_solve = h->map_epoch;
    // Behind an overlapped batch the host has not checked yet (or batches journalled for a re-run): a plain launch's tail must not
    // write the mean from partials of an expired wait either (flush_tail does the same) -- see raise_wait_expired
    d.r.err_dev = (h->d_flags && (h->overlap_used || !h->journal.empty())) ? 1 : 0;
    if (int rc = stage_state(h, p, states, states_where)) return rc;
    if (int rc = stage_noise(h, p, eps, noise, &c.mode)) return rc;
    if (int rc = check_shard_order(h, shard_rollout)) return rc;
    Prof prof;
    if (int rc = prof_begin(h, !shard_rollout && (h->pipelined || h->ticket_mode), &prof)) return rc;
    h->last_eps = p.eps;
    h->last_mode = c.mode;
    rotate_slots(h, p, d);
    if (h->arm_state_snap) { p.state_snap = h->d_state_snaps + h->snap_slot * (size_t)p.B * 3; h->arm_state_snap = false; d.r.state_snap = 1; }
    d.r.call = shard_rollout ? kCallShard : (overlap ? kCallBatchMember : kCallSolve);
    d.r.eps_mode = c.mode;
    d.r.u_buf = p.U ? 0 : -1;
    if (h->pipelined && !shard_rollout) return solve_pipelined(h, p, c, d, prof);
    if (!(h->ticket_overlap && overlap && !shard_rollout)) h->prev_published = false;
    if (p.slip_on && !h->slip_std_set) return fail(BN_ERR_STATE, "bn_mppi_set_slip_std must precede solve in sampled-slip mode");
    if (h->ticket_mode && !shard_rollout) return solve_ticket(h, p, c, d, prof);
    return solve_two_launches(h, p, c, d, prof);
}

// ---- batches ---------------------------------------------------------------------------------------------------------------------

namespace {

// Every 64 launches of a batch: how many solves has the device finished (the tails post the first action with the solve's index), and when.
// Two samples that both found the device behind the host give a cadence; anything else says nothing.
void tune_sample(bn_mppi *h)
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

// The arguments of bn_mppi_solve_n_async.
struct Batch {
    int32_t n; const float *states; bn_mem_kind states_where; const float *eps; bn_noise_kind noise; int32_t eps_ring; int64_t eps_stride;
    const float *eps_of(int32_t i) const { return eps ? eps + (size_t)(i % eps_ring) * (size_t)eps_stride : nullptr; }
    bool replayable() const { return states_where == BN_MEM_DEVICE && noise != BN_NOISE_HOST_KT2; }
    bn_mppi::BatchRec rec() const { return bn_mppi::BatchRec{n, states, eps, noise, eps_ring, eps_stride, false, nullptr}; }
};

// Overlapped launches.  Solve i+1 needs only the softmin partials of solve i, yet in one stream it also waits for solve i's
// kernel to drain and for the dispatch of its own (~2.4 us of a 13 us step).  With the latency kernel consecutive solves
// alternate between the handle's stream and a second one: solve i+1 is dispatched while solve i runs, stages its window and
// draws its first noise, and then waits on a device counter for solve i's partials (published as device-scope stores by
// the workgroups themselves).  At most two launches are in flight (each stream serialises its own); per-solve buffers
// rotate over three slots so that what a launch overwrites was last read by a launch that has completed on its stream;
// the tails (aux workgroups) are ordered by a second counter.  Results are bit-identical to the one-stream chain.
// Device-side episodes overlap the same way (role kernel): the successor reads the state its predecessor advanced with
// device-scope loads after its wait (64 instances: 29.6 -> 24.8 us per control step).
bool batch_may_overlap(const bn_mppi *h, const Batch &b)
{
    return (h->lat_kernel || h->role_overlap || h->ticket_overlap) && h->n_streams > 1 && (h->d_Xalt[0] || h->p.lean) && b.n >= 3 && b.states_where == BN_MEM_DEVICE &&
           b.noise != BN_NOISE_HOST_KT2 && !(h->cfg.flags & (BN_FLAG_PROFILE | BN_FLAG_NO_OVERLAP)) && !h->shard_pending && !h->overlap_off;
}

// Which mode this batch runs in (*mode: 0 overlapped, 1 one stream): the handle's choice, or -- for its first 192 launches, once --
// the other one, for a look (tune_record).  Returns the length of the prefix to run that way as a batch of its own, 0 when the batch
// is not split (then *mode is the whole batch's).
int32_t explore_prefix(const bn_mppi *h, bool overlap, const Batch &b, int *mode)
{
    *mode = overlap ? h->tune.chosen : 1;
    if (!(overlap && h->tune.explore && b.n >= 128 && !h->in_episode && !h->replaying)) return 0;
    const int32_t ring = b.eps ? b.eps_ring : 1;
    const int32_t prefix = ((192 + ring - 1) / ring) * ring;       // (a whole number of turns of the caller's noise ring: the rest starts at block 0 again)
    if (b.n > prefix + 2) return prefix;
    *mode = 1 - h->tune.chosen;
    return 0;
}

// May this handle's batch overlap on its device now?  See g_overlap_owner: no other handle's overlapped batch in flight, every other
// handle idle, and the two size rules.  *mine: yes, and the handle owns the device from here on.
int claim_device_for_overlap(bn_mppi *h, bool *mine)
{
    *mine = true;
    BN_BIND(h);
    std::lock_guard<std::mutex> lock(g_overlap_mu);
    bn_mppi *&owner = g_overlap_owner[h->cfg.device_id];
    if (owner && owner != h) {                      // is the owner's latest overlapped batch still in flight?
        bool busy = hipStreamQuery(owner->stream) != hipSuccess;
        for (int q = 0; !busy && q + 1 < owner->n_streams; ++q) busy = hipStreamQuery(owner->xstream[q]) != hipSuccess;
        (void)hipGetLastError();
        if (busy) *mine = false;
    }
    for (bn_mppi *o : g_handles[h->cfg.device_id]) {   // ... and is every other handle idle?  (see g_handles)
        if (!*mine) break;
        if (o == h) continue;
        for (int q = 0; *mine && q < kMaxStreams; ++q) {            // (incl. the second private stream of a host-paced handle)
            const hipStream_t os = q ? o->xstream[q - 1] : o->stream;
            if ((q && !os) || os == h->stream) continue;
            if (hipStreamQuery(os) != hipSuccess) *mine = false;
        }
    }
    (void)hipGetLastError();
    const size_t slots = residency_slots(h), wgs = (size_t)h->p.B * (h->p.nblk + 1);
    if (*mine && 2 * wgs > slots && !own_device_for_big_overlap(h->cfg.device_id)) *mine = false;
    // A launch that needs well over one residency round by itself is never fully placed while it runs: its successor's waiting
    // workgroups compete with its OWN remaining ones for every slot that frees up, whatever the host orders.  Up to a quarter over
    // (64 instances of K = 1024: 1088 workgroups on 1024 slots; 70: 1190) the remainder is placed when the first round drains and
    // nothing has ever expired (tens of thousands of launches, fresh processes included); at one and a half rounds (3 instances of
    // K = 8192 at one workgroup per CU: 387 on 256) the first batch of a fresh process expired every time (round 4,
    // tests/differential.py `ops` seed 2681).  Such batches run on one stream.
    if (*mine && 4 * wgs > 5 * slots) *mine = false;
    if (*mine) owner = h;
    else if (!owner) g_overlap_owner.erase(h->cfg.device_id);      // (operator[] above created an empty entry)
    g_overlap_owners.store((int)g_overlap_owner.size(), std::memory_order_relaxed);
    return BN_OK;
}

int solve_n_one_stream(bn_mppi *h, const Batch &b, bool overlap)
{
    h->last_batch_overlapped = false;
    for (int32_t i = 0; i < b.n; ++i) {
        if (int rc = solve_impl(h, b.states, b.states_where, b.eps_of(i), b.noise, false)) return rc;
        if (overlap && (i & 63) == 63) tune_sample(h);
    }
    if (!h->in_episode) journal_push(h, b.rec(), b.replayable());   // behind an overlapped batch not yet checked: lost with it, re-run with it
    return BN_OK;
}

// Is the handle's stream idle when the batch starts?  If not, the extra streams start behind everything enqueued so far -- or, for
// launches big enough to crowd each other out, the host waits for the stream first.
// The scheme relies on a launch having been dispatched before its successor becomes eligible: waiting workgroups hold their
// slots, and the hardware does not share freed slots fairly between two queues (seen with two 70-instance launches made
// eligible at the same instant: the successor's waiting workgroups took every slot, the predecessor's never got one, the
// waits expired).  Inside a batch that holds by construction -- launch i+1 becomes eligible when launch i-1 completes, a whole
// kernel after launch i did.  At the START it holds when the stream is idle (solve 1 is enqueued microseconds after solve 0
// went out); if earlier work is still pending, solves 0 and 1 would become eligible together, so launches big enough to
// crowd each other out wait for the stream first.
int fork_batch_streams(bn_mppi *h, bool crowd, bool *idle)
{
    *idle = hipStreamQuery(h->stream) == hipSuccess;
    (void)hipGetLastError();
    if (!*idle && crowd) {
        BN_HIP(hipStreamSynchronize(h->stream));
        *idle = true;
    }
    if (!*idle) {                                                   // fork: the extra streams start behind everything enqueued so far
        BN_HIP(hipEventRecord(h->ev_fork, h->stream));              // (nothing is: no event packet in front of the first launches)
        for (int q = 0; q + 1 < h->n_streams; ++q) BN_HIP(hipStreamWaitEvent(h->xstream[q], h->ev_fork, 0));
    }
    return BN_OK;
}

// Stream (and trajectory buffer) of solve i: round robin, except that the LAST solve always runs on the handle's own stream
// -- whatever follows it there (the batch's tail kernel, a getter) is then ordered by the queue itself instead of by a
// cross-queue event that has only just fired (measured: 18 us between the last rollout kernel and the tail).  With an
// even n the last two solves share the stream, which costs one overlap.  (Not the first two: the solve on the other
// stream would then become eligible before its predecessor is even dispatched -- see the note on eligibility above.)
// On an idle stream nothing ties the first solve to the handle's stream, so the round robin is simply aligned to END there.
inline int stream_of_solve(int32_t i, int32_t n, int S, bool idle)
{
    return idle ? (n - 1 - i) % S : (i == n - 1 ? 0 : i % S);
}

int stamp_seen(bn_mppi *h, int word, int stamp, hipStream_t wait_out)
{
    const auto t0 = std::chrono::steady_clock::now();
    while (__atomic_load_n(&h->h_err[word], __ATOMIC_ACQUIRE) != stamp) {
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) {      // something else holds the GPU: wait the launch out
            BN_HIP(hipStreamSynchronize(wait_out));
            break;
        }
    }
    return BN_OK;
}

// A launch that exceeds one residency round (up to 1.25 rounds overlap at all, see claim_device_for_overlap): a launch whose workgroups
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
// Called in front of launch i (< 3) of such a batch; `qs` is its stream, *stamp the batch's marker value (set at i == 0).
int hand_over_first_launches(bn_mppi *h, int32_t i, hipStream_t qs, int *stamp)
{
    const int S = h->n_streams;
    if (i == 0) {
        *stamp = (int)(h->solves & 0x3fffffff) + 1;
        for (int w = 4; w < 8; ++w) __atomic_store_n(&h->h_err[w], 0, __ATOMIC_RELEASE);
        if (S > 1) BN_HIP(bn::launch_stamp(h->d_err + 5, *stamp, h->xstream[0]));      // wakes the other queue
        BN_HIP(bn::launch_stamp(h->d_err + 4, *stamp, qs));
    } else if (i == 1) {
        if (int r = stamp_seen(h, 4, *stamp, h->stream)) return r;                         // the first launch is next in a queue that is being processed
        if (S > 1) { if (int r = stamp_seen(h, 5, *stamp, h->xstream[0])) return r; }
        BN_HIP(bn::launch_stamp(h->d_err + 6, *stamp, qs));
    } else {
        if (int r = stamp_seen(h, 6, *stamp, h->xstream[0])) return r;                     // ... and so is the second
    }
    return BN_OK;
}

// The end of an overlapped batch: its tail, the experimental join, its journal record.
int finish_batch(bn_mppi *h, const Batch &b, int rc)
{
    // A long batch ends with its own tail, enqueued right behind the last solve and BEFORE the join: a tail kernel that comes later
    // (flush, sync, a getter) would sit behind the join's barrier packet, ~10 us of queue processing after the last rollout kernel.
    // Short batches keep the tail pending: chained short batches carry it in their next launch for free.
    if (rc == BN_OK && b.n >= kEagerTailMinBatch && !h->in_episode) rc = flush_tail(h);
    static const bool exp_join = exp_env("BN_JOIN") != nullptr;   // experiments (tools/region_overhead.py)
    for (int q = 0; exp_join && q + 1 < h->n_streams; ++q) {        // join: the handle's stream continues behind all of them
        hipError_t e1 = hipEventRecord(h->ev_join[q], h->xstream[q]);
        hipError_t e2 = hipStreamWaitEvent(h->stream, h->ev_join[q], 0);
        if (rc == BN_OK && (e1 != hipSuccess || e2 != hipSuccess)) rc = fail(BN_ERR_HIP, "joining the overlapped launches failed");
    }
    if (rc == BN_OK && !h->in_episode) journal_push(h, b.rec(), b.replayable());
    return rc;
}

int solve_n_overlapped(bn_mppi *h, const Batch &b)
{
    BN_BIND(h);
    h->last_batch_overlapped = true;
    if (!h->replaying && h->journal.empty() && !h->journal_lost) {   // first batch since the error word was last seen clean
        h->journal_solves0 = h->solves;
        h->arm_snap = true;
    }
    const int S = h->n_streams;
    const size_t slots = residency_slots(h), wgs = (size_t)h->p.B * (h->p.nblk + 1);
    // Launches big enough to crowd each other out start on the handle's OWN stream, whatever that costs at the batch's end.  Aligning
    // the round robin to end there puts solve 0 of an even batch on the internal stream -- a queue that has been idle since the last
    // batch and wakes up later than the handle's, which has just carried the caller's work: solve 1 was then dispatched BEFORE solve 0,
    // its waiting workgroups took the slots solve 0 needed, and the bounded waits expired (round 4, tools/_seq tests: 3-7 of 18 fresh
    // 64-instance handles with even batch lengths, none with odd ones; it is what made test_big_batches_... fail one run in eight).
    const bool crowd = 2 * wgs > slots;
    bool idle = false;
    if (int rc = fork_batch_streams(h, crowd, &idle)) return rc;
    // The last launch of a long batch carries its own tail as a second aux workgroup (SolveParams::self_tail; the one-launch kernel,
    // rollout_lat.inc mode 1) instead of a tail kernel behind it: since round 6 that workgroup stages its window while the rollouts run
    // and polls the granules of their rows -- 3 us off a 20-solve region (tools/region_ab.py: 215.2 -> 212.2 us; the counter-waiting
    // tail of rounds 2-5 had measured 5 us WORSE than the kernel behind).  BN_NO_SELF_TAIL (experiment builds) turns it off.
    const bool exp_self_tail = exp_env("BN_NO_SELF_TAIL") == nullptr;      // (read per batch: tools/region_ab.py toggles it inside one process)
    static const bool exp_align = exp_env("BN_NO_ALIGN") == nullptr;
    if (!exp_align) idle = false;                                   // (only the stream assignment below looks at it from here on)
    if (crowd && !exp_env("BN_ALIGN_BIG")) idle = false;      // (BN_ALIGN_BIG: tools/recovery_stress.py brings the race back)
    // Only launches that exceed one residency round by THEMSELVES can be starved for good (a waiting launch of at most one round
    // leaves its predecessor's running workgroups to finish and free what the rest of it needs): two launches that merely do not
    // fit side by side -- 256 instances on the one-wave kernel, K = 16384 -- skip the hand-over.
    const bool hand_over = wgs > slots && !h->replaying && b.n >= 3;
    int rc = BN_OK;
    int stamp = 0;
    for (int32_t i = 0; i < b.n && rc == BN_OK; ++i) {
        const int q = stream_of_solve(i, b.n, S, idle);
        // A long batch ends with its own tail (see finish_batch): on the latency kernel it rides in the last launch as a second aux workgroup.
        const bool own_tail = i == b.n - 1 && b.n >= kEagerTailMinBatch && exp_self_tail;
        if (hand_over && i < 3) {
            if (int r = hand_over_first_launches(h, i, launch_stream(h, q), &stamp)) return r;
        }
        rc = solve_impl(h, b.states, b.states_where, b.eps_of(i), b.noise, false, true, q, own_tail);
        if ((i & 63) == 63) tune_sample(h);
    }
    return finish_batch(h, b, rc);
}

}  // namespace

}  // namespace host
}  // namespace bn

using namespace bn::host;

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
    const Batch b{n, states, states_where, eps, noise, eps_ring, eps_stride};
    const bool overlap = batch_may_overlap(h, b);
    int mode = 1;
    if (const int32_t prefix = explore_prefix(h, overlap, b, &mode)) {
        if (int rc = bn_mppi_solve_n_async(h, prefix, states, states_where, eps, noise, eps_ring, eps_stride)) return rc;
        h->tune.explore = 0;                                        // (looked, whether or not the windows were conclusive)
        return bn_mppi_solve_n_async(h, n - prefix, states, states_where, eps, noise, eps_ring, eps_stride);
    }
    if (mode != h->run_mode) h->ov_sample.valid = false;
    h->run_mode = mode;
    bool mine = overlap && mode == 0;
    if (mine) {
        if (int rc = claim_device_for_overlap(h, &mine)) return rc;
    }
    if (b.replayable() && !h->in_episode) journal_arm_states(h);
    return mine ? solve_n_overlapped(h, b) : solve_n_one_stream(h, b, overlap);
}

int bn_mppi_solve(bn_mppi_t *h, const float *states, bn_mem_kind states_where, const float *eps,
                  bn_noise_kind noise, float *ustar_host, float *xstar_host)
{
    if (!h) return fail(BN_ERR_INVALID, "null handle");
    BN_BIND(h);
    if (int rc = settle_point(h)) return rc;
    if (h->lat_kernel && h->tail_pending && !h->self_off) { if (int rc = flush_tail(h)) return rc; }      // (as in forward_impl)
    if (int rc = solve_impl(h, states, states_where, eps, noise, false, false, 0, true)) return rc;   // own tail in the launch where that exists
    if (int rc = flush_tail(h)) return rc;
    const size_t B = h->p.B, T = h->p.T;
    if (ustar_host) BN_HIP(hipMemcpyAsync(ustar_host, h->d_ustar, B * T * 2 * 4, hipMemcpyDeviceToHost, h->stream));
    if (xstar_host)
        BN_HIP(hipMemcpyAsync(xstar_host, h->d_xstar, B * (T + 1) * 3 * 4, hipMemcpyDeviceToHost, h->stream));
    BN_HIP(hipStreamSynchronize(h->stream));
    return self_check(h);
}

// Test hook: the launch log (log_launch, mppi_launch.h).  A ring of kLaunchLogCap records: what was not read in time is overwritten.
int bn_mppi_debug_launch_log(bn_mppi_t *h, bn_mppi_launch_record *out, int32_t cap)
{
    if (!h) return fail(BN_ERR_INVALID, "null handle");
    if (!out) {                                        // on, and empty
        h->launch_log.assign(kLaunchLogCap, bn_mppi_launch_record{});
        h->log_head = h->log_read = 0;
        h->log_on = true;
        return 0;
    }
    if (!h->log_on || cap < 0) return fail(BN_ERR_INVALID, "the launch log is off (call with out == NULL first), or cap < 0");
    if (h->log_head - h->log_read > kLaunchLogCap) h->log_read = h->log_head - kLaunchLogCap;
    int32_t n = 0;
    while (h->log_read < h->log_head && n < cap) out[n++] = h->launch_log[h->log_read++ % kLaunchLogCap];
    return n;
}

}  // extern "C"
