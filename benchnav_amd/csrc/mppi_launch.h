// mppi_launch.h -- what every launch of the solve path is made from (mppi_solve.cpp, flush_tail in mppi_capi.cpp, hp_prelaunch in
// mppi_paced.cpp): the layout of the counter block d_flags, the slot rotation of the per-solve buffers, the launch decision -- what a
// launch will be, as plain numbers and buffer identities, settled before anything is enqueued -- and its application: the pointers of
// SolveParams, the host mirrors of the device counters, the launch log, the launch.  Private, host only, not installed.
#pragma once
#include "mppi_handle.h"

#include <algorithm>

namespace {

// ---- d_flags: [kSlots][B] part counters | [B] tail counters | a spare slot | the device error word, kFlagStride counters apart ------
inline size_t flag_word(size_t B, size_t i) { return ((kSlots + 1) * B + i) * bn::kFlagStride; }      // word i behind the [kSlots + 1][B] counters
inline size_t flag_bytes(size_t B) { return flag_word(B, 3) * sizeof(unsigned long long); }
inline unsigned long long *flag_part(const bn_mppi *h) { return h->d_flags; }
inline unsigned long long *flag_tail(const bn_mppi *h) { return h->d_flags + kSlots * (size_t)h->p.B * bn::kFlagStride; }
inline unsigned long long *spare_counter(const bn_mppi *h) { return h->d_flags + flag_word(h->p.B, 1); }      // zero between its users
inline int *err_dev(const bn_mppi *h) { return reinterpret_cast<int *>(h->d_flags + flag_word(h->p.B, 2)); }     // see raise_wait_expired

// Workgroups of the handle's kernel family the device holds at once: what "two launches fit side by side" is measured against.
inline size_t residency_slots(const bn_mppi *h)
{
    return h->wave_kernel ? 24 * (size_t)std::max(h->n_cus, 1) : (h->lat_kernel ? (size_t)std::max(h->n_cus, 1) : h->resident_wgs);
}

// A synchronous solve on the latency kernel with its own tail in the launch: it publishes like a member of a batch (counters, granules)
// -- for its OWN tail, the second aux workgroup of the same launch; it waits for nobody (no predecessor in flight, no tail pending: the
// callers see to that).
inline bool lone_self_solve(const bn_mppi *h, bool self_tail, bool overlap)
{
    return self_tail && !overlap && h->lat_kernel && !h->in_episode && !h->tail_pending && !h->replaying && !h->self_off &&
           !(h->cfg.flags & BN_FLAG_NO_PIPELINE);
}

enum LaunchCall { kCallSolve = 0, kCallBatchMember = 1, kCallTail = 2, kCallPrelaunch = 3, kCallShard = 4 };
enum LaunchEntry { kRollout = 0, kRolloutLatSelf = 1, kRolloutLatHost = 2, kRolloutLatHostRef = 3, kRolloutSampled = 4, kFinish = 5 };

// What one launch will be.  `r` is what the kernel will see and which launch function takes it (the launch log shows it as it is,
// include/benchnav_mppi.h); the rest is what the host books beside it.  Decided from the handle's state without changing it.
struct LaunchDecision {
    bn_mppi_launch_record r{};
    int cur = 0, prev = 0;               // slots of this solve's and the previous solve's per-solve buffers (r.cur_slot / r.prev_slot: only where the kernel looks)
    unsigned long long publish = 0;      // the launch counts this into flag_part[cur]: its rollout workgroups (nblk), or its ticket merge (1)
    int tails = 0;                       // tails the launch writes and counts into flag_tail: the previous solve's, its own
    bool member = false;                 // of an overlapped batch
    bool lone_self = false;
};

inline hipStream_t launch_stream(const bn_mppi *h, int index) { return index ? h->xstream[index - 1] : h->stream; }      // (hp_stream[q] is xstream[q])

// Per-solve buffers: kSlots slots, solve i uses slot i % kSlots (bn_mppi::d_cost).
inline void rotate_slots(const bn_mppi *h, bn::SolveParams &p, LaunchDecision &d)
{
    d.cur = (int)(h->solves % kSlots); d.prev = (int)((h->solves + kSlots - 1) % kSlots);
    p.solve = d.r.solve = h->solves;
    p.part = h->d_part[d.cur]; p.cost = h->d_cost[d.cur]; p.state_copy = h->d_state_copy[d.cur];
    p.part_prev = h->d_part[d.prev]; p.cost_prev = h->d_cost[d.prev]; p.state_prev = h->d_state_copy[d.prev];
}

// Member of an overlapped batch: the launch publishes into its slot -- `publish` counts per instance: its rollout workgroups, or one for
// the ticket merge -- and waits on the device if its predecessor published; `granules`: the rows travel as granule copies too.
inline void join_batch(const bn_mppi *h, LaunchDecision &d, int q, unsigned long long publish, bool granules)
{
    bn_mppi_launch_record &r = d.r;
    r.flag_part = r.err = r.err_dev = 1;               // (err: pinned host memory, mapped)
    r.mean_snap = h->arm_snap ? 1 : 0;
    r.cur_slot = d.cur; r.prev_slot = d.prev;
    r.wait_part = h->pub[d.prev];
    r.gran = (granules && h->d_gran[d.cur]) ? 1 : 0;
    if (q) {                                           // this solve's trajectories / controls go to one of the extra buffers
        if (h->d_Xalt[q - 1]) r.x_buf = q;
        if (h->d_Ualt[q - 1] && r.u_buf >= 0) r.u_buf = q;
    }
    r.overlap = (h->prev_published && r.have_prev) ? 1 : 0;
    r.gran_prev = (r.overlap && granules && h->d_gran[d.prev]) ? 1 : 0;
    r.stream = q;
    d.publish = publish;
    d.member = true;
}

// The launch carries its own tail as a second aux workgroup: it waits on the device for the rollout workgroups of its own launch and for
// every tail before it.  After what the launch publishes and the tail of the previous solve it may carry have been decided.
inline void carry_own_tail(const bn_mppi *h, LaunchDecision &d)
{
    d.r.self_tail = 1;
    d.r.wait_part_self = h->pub[d.cur] + d.publish;
    d.r.wait_tail_self = h->tails + (unsigned long long)d.tails;
    d.tails += 1;
}

inline void log_launch(bn_mppi *h, const bn_mppi_launch_record &r)
{
    if (__builtin_expect(!h->log_on, 1)) return;
    h->launch_log[h->log_head++ % h->launch_log.size()] = r;
}

// The scalars and the pointers a decision stands for.
inline void fill_params(const bn_mppi *h, bn::SolveParams &p, const LaunchDecision &d)
{
    const bn_mppi_launch_record &r = d.r;
    p.tail_solve = r.tail_solve;
    p.have_prev = r.have_prev; p.mean_from_part = r.mean_from_part; p.self_tail = r.self_tail; p.overlap = r.overlap;
    p.cur_slot = r.cur_slot; p.prev_slot = r.prev_slot;
    p.wait_part = r.wait_part; p.wait_tail = r.wait_tail; p.wait_part_self = r.wait_part_self; p.wait_tail_self = r.wait_tail_self;
    p.wave_kernel = r.wave_kernel; p.lat_kernel = r.lat_kernel; p.aux_prio = r.aux_prio; p.tail_merged = r.tail_merged;
    p.closed_loop = r.closed_loop; p.env_on = r.env_on; p.ep_index = r.ep_index; p.host_paced = r.host_paced;
    if (r.x_buf) p.X = h->d_Xalt[r.x_buf - 1];
    p.U = r.u_buf < 0 ? nullptr : (r.u_buf ? h->d_Ualt[r.u_buf - 1] : p.U);
    p.flag_part = r.flag_part ? flag_part(h) : nullptr;
    p.flag_tail = r.flag_tail ? flag_tail(h) : nullptr;
    p.gran = r.gran ? h->d_gran[d.cur] : nullptr;
    p.gran_prev = r.gran_prev ? h->d_gran[d.prev] : nullptr;
    p.err = r.err ? h->d_err : nullptr;
    p.err_dev = r.err_dev ? err_dev(h) : nullptr;
    if (r.mean_snap) p.mean_snap = h->d_mean_snap;
    if (r.out_copy_self) p.out_copy_self = h->self_out_copy;
    if (r.env_z) p.env_z = h->ep_z + (size_t)r.ep_index * p.B;
    if (r.state_inline) { p.state_inline = 1; p.sv0 = h->inline_state[0]; p.sv1 = h->inline_state[1]; p.sv2 = h->inline_state[2]; }
}

// The host mirrors of what the launch counts on the device, and what it used up.  hp_cancel (mppi_handle.h) undoes the two counters
// for a prelaunch that is told to leave.
inline void advance_mirrors(bn_mppi *h, const LaunchDecision &d)
{
    if (d.r.mean_snap) h->arm_snap = false;
    if (d.r.overlap && d.member) h->overlap_used = true;
    h->pub[d.cur] += d.publish;
    h->tails += (unsigned long long)d.tails;
}

// A solve's launch: both, in front of the launch -- as the mirrors of a solve have always been advanced.  (hp_prelaunch advances them
// behind a launch that succeeded.)
inline void apply_decision(bn_mppi *h, bn::SolveParams &p, const LaunchDecision &d)
{
    fill_params(h, p, d);
    advance_mirrors(h, d);
    log_launch(h, d.r);
}

}  // namespace
