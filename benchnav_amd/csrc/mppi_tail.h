// mppi_tail.h -- the tail of a solve (finish_body), step by step, and the layout of its LDS, which the host sizes from as well.
#pragma once
#include "mppi_stamps.h"
#include "mppi_geometry.h"
#include "mppi_chain.h"
#include "mppi_env_step.h"
#include "mppi_slip.h"
#include "mppi_sync.h"
#include "mppi_merge.h"

namespace bn {

namespace {

// The LDS of a tail, in floats:
//   [ window WN x WN | us: U* 2T | xl: X* 3(T+1) | sc: scale nblk | red kRedFloats | group rows ceil(nblk/16) x (2+2T) if 64 < nblk <= 1024
//     (merge_partials puts them behind red) | sampled slip: zol, the draws of X* | win2: the (mean, std) window 2 x WN x WN ]
// finish_body carves it up with a pointer chain of its own (us, xl, sc, red, zol, win2) and tail_lds_floats adds up the size the host
// asks for (finish_lds_bytes).  The terms of the sum are the functions below, and BOTH sides call them: the chain (I = int) and the
// total (I = size_t) cannot drift apart term by term.  (An offset table that the chain reads its pointers from changed the code of
// every tail: profiles/mppi_device_split.txt.)
template <typename I> __host__ __device__ __forceinline__ constexpr I tail_window_floats(I WN) { return WN * WN; }
template <typename I> __host__ __device__ __forceinline__ constexpr I tail_ustar_floats(I T) { return 2 * T; }
template <typename I> __host__ __device__ __forceinline__ constexpr I tail_xstar_floats(I T) { return 3 * (T + 1); }
// the group rows of the two-level merge (PS = 2 + 2T floats a row), none outside its range
template <typename I> __host__ __device__ __forceinline__ constexpr I tail_group_floats(I nblk, I PS)
{
    return (nblk > 64 && nblk <= 64 * kGroupRows) ? ((nblk + kGroupRows - 1) / kGroupRows) * PS : 0;
}
// from zol to win2 (before its alignment): the draws come in blocks of four, one block past the last step's
template <typename I> __host__ __device__ __forceinline__ constexpr I tail_draw_floats(I T) { return (T + 7) & ~(I)3; }

// The sampled-slip part is T + kSlipSlack + 2 WN^2 floats, as it always was; the slack by name:
constexpr int kSlipRoundT = 3;      // T rounded up to whole blocks of four draws: at most three more
constexpr int kSlipBlock = 4;       // ... and one block more
constexpr int kSlipAlignWin2 = 1;   // the kernel rounds win2 up to an 8-byte ADDRESS: at most one float
constexpr int kSlipPad = 8;         // unused
constexpr int kSlipSlack = kSlipRoundT + kSlipBlock + kSlipAlignWin2 + kSlipPad;
static_assert(kSlipSlack == 16, "the size of a tail's LDS is part of the plan (tests/test_mppi_plan.py)");
static_assert(tail_draw_floats(48) == 48 + kSlipBlock && tail_draw_floats(49) == 49 + kSlipRoundT + kSlipBlock, "the draws' share of the slack");

inline size_t tail_lds_floats(size_t WN, size_t T, size_t nblk, bool slip)      // WN = 0 without the LDS window
{
    size_t n = tail_window_floats(WN) + tail_ustar_floats(T) + tail_xstar_floats(T) + nblk + kRedFloats + tail_group_floats(nblk, 2 + 2 * T);
    if (slip) {
        const size_t draws = tail_draw_floats(T);
        const size_t spare = T + kSlipRoundT + kSlipBlock - draws;       // what the rounding of T did not take
        n += draws + kSlipAlignWin2 + 2 * tail_window_floats(WN) + spare + kSlipPad;
    }
    return n;
}

// the environment step that follows this solve: apply U*[0], log state, reward and goal arrival
template <int GEO, bool AGENT>
__device__ __forceinline__ void tail_env_step(const SolveParams &p, int b, float sx, float sy, float sth, const float *us)
{
    const EnvStep e = env_advance<GEO>(p, b, sx, sy, sth, us[0], us[1], p.env_z, (uint64_t)p.ep_index);
    const size_t B = p.B;
    float *row = p.ep_states + ((size_t)(p.ep_index + 1) * B + b) * 3;
    row[0] = e.x; row[1] = e.y; row[2] = e.th;
    st<AGENT>(p.env_state + b * 3 + 0, e.x); st<AGENT>(p.env_state + b * 3 + 1, e.y); st<AGENT>(p.env_state + b * 3 + 2, e.th);
    p.ep_reward[(size_t)p.ep_index * B + b] = e.reward;
    p.ep_action[((size_t)p.ep_index * B + b) * 2 + 0] = us[0];
    p.ep_action[((size_t)p.ep_index * B + b) * 2 + 1] = us[1];
    if (p.ep_index == 0) {
        float *row0 = p.ep_states + (size_t)b * 3;
        row0[0] = sx; row0[1] = sy; row0[2] = sth;
    }
    // (tails of consecutive solves may run in different launches in flight at once: device-scope accesses, like the mean)
    if (e.reached && !e.frozen) {
        const int seen = AGENT ? __hip_atomic_load(p.ep_done + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : p.ep_done[b];
        if (seen < 0) { if (AGENT) __hip_atomic_store(p.ep_done + b, p.ep_index, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else p.ep_done[b] = p.ep_index; }
    }
}

// _weights = softmax(-costs / lambda)   mppi.py:193, and the stable copy of the costs, by the waves behind the first of a multi-wave
// tail: rollouts tid - t0, tid - t0 + step, ..  The start stays the difference of two arguments: handed over as one value, the
// compiler knows its sign and the loop is no longer instruction for instruction the one this was; and the single-wave tail keeps
// its own copy of the loop in finish_body for the same reason (profiles/mppi_device_split.txt).
template <bool AGENT>
__device__ __forceinline__ void tail_weights(const SolveParams &p, int b, const float *cost_all, int K, float m, float S, int tid, int t0, int step)
{
    const float *cost = cost_all + (size_t)b * K;
    float *wout = p.w + (size_t)b * K;
    float *cout = p.cost_out + (size_t)b * K;
    for (int k = tid - t0; k < K; k += step) {
        const float ck = ld<AGENT>(cost + k);
        st<AGENT>(cout + k, ck);
        st<AGENT>(wout + k, expf((-ck) / p.lambda_ - m) / S);
    }
}

// The tail of one solve of instance b: U* (and the next mean), softmin statistics, normalised weights,
// a stable copy of the costs, and the batch-1 rollout X* of U*.  NT threads (320 as the aux workgroup, 1024 stand-alone for large K).
// LDS: [ window | ustar 2T | X* 3(T+1) | scale nblk | red 32 | group rows ceil(nblk/16) x (2+2T) if nblk > 64 | sampled mode: draws, (mean, std) window ]
// AGENT: the launch overlaps its predecessor (other stream): wait for the counters first, read what the predecessor wrote with
// device-scope loads, and write EVERY output with device-scope (sc1, write-through) stores: the tails of consecutive solves run in
// different kernels, possibly on different XCDs, and write the same addresses -- the tail counter orders the stores themselves, but
// a plain store may sit dirty in its XCD's L2 until its kernel ends, and which kernel ends last is not ordered by anything.
// SELF (round 6): the tail of the solve whose rollouts run in THIS launch (SolveParams::self_tail) -- a synchronous forward() as one
// launch, or the last launch of a batch.  Nothing it needs before the rows is unknown: the state is the caller's (or travels in the kernel
// arguments), so the window is staged and in LDS long before the rollout workgroups are through.  With `gran_self` (the granule copies of
// this solve's partial rows, K <= 1024) every thread then polls the granules IT merges -- one memory round trip from "stored" to "merged",
// no counter, no second fetch -- and thread 0 posts U*[0] to the host's mailbox the moment the merge is done.  The costs travel as plain
// device-scope stores, not as granules: the waves that turn them into weights wait for the workgroups' counts (publish_counter: every
// store acknowledged) first, off the critical path.  Without granules: the counter, then the rows (as AGENT).
template <int GEO, bool LDSWIN, int NT, bool BIG = false, bool AGENT = false, bool WIDE = false, bool REF = false, bool SELF = false>
__device__ __forceinline__ void finish_body(const SolveParams &p, int b, const float *part_all, const float *cost_all,
                                            const float *state_all, float *smem, const unsigned long long *gran_self = nullptr)
{
    static_assert(!SELF || AGENT, "the tail of a launch's own solve reads what the rollout workgroups of that launch publish");
    // Tails of consecutive overlapped solves write the same output buffers, so they are ordered by a counter.  What has to be ordered are
    // the STORES: with the wait in front of everything (rounds 3-4) a tail started when its predecessor was through, and at ~8.5 us a
    // tail (two dependent fetches, the merge, the 50-step rollout of U*) the chain of tails, not the rollouts, set the period of a batch
    // of dependent solves (tools/block_trace_lat.py: the aux workgroup left its launch 4 us after the rollout workgroups).  Open loop,
    // the waves that write (1 ..) wait for the tail before this one just before their first store, behind the merge; wave 0 rolls U*
    // out into LDS meanwhile and meets them at the barrier in front of its own stores.  (Episodes: the environment step reads what the
    // previous tail wrote -- the wait stays in front.)
    // (Reference order: its tail -- a sine and a cosine per step of the serial rollout -- is as long as its period; with the window
    // staged early, below, the deferred wait brings it from 11.05 to 10.8 us per dependent solve.  Alone it had measured 13.1 against
    // 11.5: the phase between the successor's polls and the publication, DESIGN_NOTEBOOK.md R5.4.)
    const bool defer_tail_wait = AGENT && NT > 64 && !p.env_on && !p.slip_on && !p.tail_merged;
    // Reference order, whose tail is as long as its period: while the solve whose
    // tail this is still runs, the window is staged around the state as it reads NOW -- two dependent fetches that were the first
    // 1.4 us of the tail after the rows: 11.5 -> 10.9 us per dependent solve.  The state is written early in that solve's prologue
    // and almost always there; a thread that read something else (checked below against the load behind the wait) stages its cells
    // again.  (The default arithmetic's period is the rollouts' path and its instantiation is left exactly as it was: the same
    // lines there -- even as dead code that only moved declarations -- measured 7.93 -> 8.11 us.)
    float sx0 = 0.0f, sy0 = 0.0f;
    bool staged = false;
    if constexpr (AGENT && REF && LDSWIN && !SELF) {
        if (!p.slip_on && !p.env_on) {
            sx0 = ld<AGENT>(state_all + b * 3 + 0); sy0 = ld<AGENT>(state_all + b * 3 + 1);
            stage_window(smem, p.map + (size_t)b * p.map_stride, window_origin<GEO>(p, sx0, sy0), p.WN, p.G, (int)threadIdx.x, NT);
            staged = true;
        }
    }
    const bool self_gran = SELF && gran_self != nullptr && !p.tail_merged;
    if (AGENT && !SELF) {
        if (threadIdx.x == 0) {
            wait_counter(flag_ctr(p.flag_part, p.prev_slot * p.B + b), p.wait_part, p);   // the solve whose tail this is has published everything
            if (!defer_tail_wait) wait_counter(flag_ctr(p.flag_tail, b), p.wait_tail, p);   // and the tail before it has left the output buffers
        }
        __syncthreads();
    }
    // p.tail_merged: U* and the softmin statistics of this solve were merged already (ticket merge of the sampled
    // kernel, which also wrote the next mean); they come from (ustar_prev, stats_prev).
    const int T = p.T, K = p.K, nblk = p.nblk, PS = 2 + 2 * p.T;
    float *win = smem;
    float *us = win + (LDSWIN ? tail_window_floats(p.WN) : 0);
    float *xl = us + tail_ustar_floats(T);                             // X* rows: the serial rollout's lane stages them here
    float *sc = xl + tail_xstar_floats(T);
    float *red = sc + nblk;

    const int tid = threadIdx.x;
    const float *__restrict__ map = p.map + (size_t)b * p.map_stride;
    const float *part = part_all + (size_t)b * nblk * PS;
    float sx, sy, sth;
    BN_SSTAMP(0);
    if constexpr (SELF) {                              // the state this launch's rollouts start from: the caller's, known from the start
        if (p.state_inline) { sx = p.sv0; sy = p.sv1; sth = p.sv2; }
        else { sx = p.state[b * 3 + 0]; sy = p.state[b * 3 + 1]; sth = p.state[b * 3 + 2]; }
    } else {
        sx = ld<AGENT>(state_all + b * 3 + 0); sy = ld<AGENT>(state_all + b * 3 + 1); sth = ld<AGENT>(state_all + b * 3 + 2);
    }
    BN_STAMP(8);

    // the merge's loads go out before the window staging (which waits for the state): one memory round trip for both
    MergeLoads pre{};
    const bool pre_ok = !p.tail_merged && nblk <= 64;
    if (pre_ok && !SELF) pre = merge_issue<AGENT>(part, nblk, T, tid);
    Win w{0, 0, 0.f, 0.f, 0.f, 0.f};
    if (LDSWIN && !p.slip_on) {
        w = window_origin<GEO>(p, sx, sy);
        if constexpr (AGENT && REF && !SELF) { if (!(staged && sx == sx0 && sy == sy0)) stage_window(win, map, w, p.WN, p.G, tid, NT); }   // (per thread: no barrier inside)
        else stage_window(win, map, w, p.WN, p.G, tid, NT);
    }
    BN_SSTAMP(1);
    if constexpr (SELF) {
        // ... and only now the wait for this launch's own rollout workgroups: they were dispatched before this workgroup (grid order) and
        // wait for nobody that comes after them, so the wait ends; it is bounded all the same (the error word, see bn_mppi_forward_async)
        if (self_gran) {
            const unsigned long long *grows = gran_self + (size_t)b * nblk * PS;
            const uint32_t tag = (uint32_t)p.tail_solve + 1u;
            const bool early = p.host_paced && !p.no_early_mail;
            if (tid < 64 && !p.have_prev && p.mail != nullptr && early) {
                // The host waits for U*[0] -- two columns of the sixteen rows.  Wave 0 polls just those (and the rows' statistics): a light
                // poll sees the rows sooner than the full one (the lines that are being written are what makes a poll slow: notebook R5.4),
                // and its lanes 0 and 1 post the first action -- merge_one: the arithmetic of merge_partials, the same bits -- before the
                // workgroup has merged anything else.  Then it joins the full poll below (the rows are there by then).  Host-paced launches
                // only (same box, C loop: 15.2 -> 14.6 us per step): the tail ends 1.2 us later for it, and a one-launch forward that is
                // called back to back waits for exactly that end (22.7 -> 23.7 us per step there).
                GranulePoll pa;
                MergeLoads L{};
                bool got = false;
                for (int it = 0; it < (1 << 21) && !got; ++it) {
                    pa.issue(grows, nblk, T, tid, tid & 1);
                    got = __builtin_amdgcn_ballot_w64(!pa.take(tag, nblk, T, tid, tid & 1, L)) == 0;
                }
                if (!got) raise_wait_expired(p, nullptr, 902);
                const float val = merge_one(L, nblk, tid);
                if (tid < 2) store_granule_host(p.mail + 2 * b + tid, val, (uint32_t)p.tail_solve + 1u);
                BN_SSTAMP(3);
            }
            bool ok = false;
            for (int it = 0; it < (1 << 22) && !ok; ++it) {
                pre = merge_issue_granules(grows, nblk, T, tid, tag, ok, tid);
                if (!ok) __builtin_amdgcn_s_sleep(1);
            }
            if (!ok) raise_wait_expired(p, nullptr, 901);
        } else {
            if (tid == 0) wait_counter(flag_ctr(p.flag_part, p.prev_slot * p.B + b), p.wait_part, p);
            __syncthreads();
            if (pre_ok) pre = merge_issue<AGENT>(part, nblk, T, tid);
        }
        if (!defer_tail_wait) {                        // (not reached by today's callers: the latency kernel's self tail always defers)
            if (tid == 0) {
                if (self_gran) wait_counter(flag_ctr(p.flag_part, p.prev_slot * p.B + b), p.wait_part, p);
                wait_counter(flag_ctr(p.flag_tail, b), p.wait_tail, p);
            }
            __syncthreads();
        }
    }
    BN_STAMP(9);
    BN_SSTAMP(2);

    float m, S;
    if (p.tail_merged) {
        for (int j = tid; j < 2 * T; j += NT) {
            const float u = ld<AGENT>(p.ustar_prev + (size_t)b * 2 * T + j);
            us[j] = u;
            if (!(BIG && p.ustar_written)) st<AGENT>(p.ustar + (size_t)b * 2 * T + j, u);      // (BIG: the stand-alone tail, the only one that follows a merge kernel)
            if (p.out_copy) st<AGENT>(p.out_copy + (size_t)b * 2 * T + j, u);
        }
        m = ld<AGENT>(p.stats_prev + b * 2 + 0);
        S = ld<AGENT>(p.stats_prev + b * 2 + 1);
        __syncthreads();
    } else {
        if constexpr (SELF) {
            // No tail in front of this one (a synchronous forward(): every earlier tail was ordered before the launch by the stream): the
            // first control goes to the host's mailbox at once -- by the two threads that merged its columns, each its own, in front of the
            // barrier the other waves' columns are waited for at -- and before the wait for the costs, the X* rollout and the weights.
            merge_partials<NT, AGENT, BIG, false, WIDE>(part, nblk, T, us, sc, red, tid, m, S, pre_ok, pre);
            if ((!self_gran || !p.host_paced || p.no_early_mail) && !p.have_prev && p.mail != nullptr && nblk <= 64 && tid < 2) store_granule_host(p.mail + 2 * b + tid, us[tid], (uint32_t)p.tail_solve + 1u);   // (self_gran: posted above)
            __syncthreads();
        } else {
            merge_partials<NT, AGENT, BIG, true, WIDE>(part, nblk, T, us, sc, red, tid, m, S, pre_ok, pre);
        }
    }
    const bool mail_early = SELF && !p.have_prev && p.mail != nullptr && (p.tail_merged || nblk <= 64);
    if (mail_early && p.tail_merged && tid == 0) {
        store_granule_host(p.mail + 2 * b, us[0], (uint32_t)p.tail_solve + 1u);
        store_granule_host(p.mail + 2 * b + 1, us[1], (uint32_t)p.tail_solve + 1u);
    }
    if (!self_gran || !p.host_paced || p.no_early_mail) BN_SSTAMP(3);
    // U*, the next mean, the statistics: threads j0, j0 + step, .. (all of them, or -- deferred wait -- the writing waves behind their wait)
    auto store_ustar = [&](int j0, int step, bool first) {
        if (!p.tail_merged) {
            const bool spoiled = batch_spoiled(p);             // a wait of this stretch expired: nothing merged since may reach `mean`
            for (int j = j0; j < 2 * T; j += step) {
                st<AGENT>(p.ustar + (size_t)b * 2 * T + j, us[j]);
                if (p.out_copy) st<AGENT>(p.out_copy + (size_t)b * 2 * T + j, us[j]);
                if (spoiled) continue;
                if (p.mean_used) st<AGENT>(p.mean_used + (size_t)b * 2 * T + j, ld<AGENT>(p.mean + (size_t)b * 2 * T + j));   // what this solve sampled around
                st<AGENT>(p.mean + (size_t)b * 2 * T + j, us[j]);  // _previous_action_seq = U*, no shift (mppi.py:217)
            }
        }
        if (first) {
            if (p.mail && !mail_early) {               // the first control of U*, for the host that waits for it: out before anything else
                store_granule_host(p.mail + 2 * b, us[0], (uint32_t)p.tail_solve + 1u);
                store_granule_host(p.mail + 2 * b + 1, us[1], (uint32_t)p.tail_solve + 1u);
            }
            st<AGENT>(p.stats + b * 2 + 0, m);
            st<AGENT>(p.stats + b * 2 + 1, S);
        }
    };
    if (!defer_tail_wait) store_ustar(tid, NT, tid == 0);
    if (p.env_on && tid == 64) tail_env_step<GEO, AGENT>(p, b, sx, sy, sth, us);
    BN_STAMP(10);

    if (p.slip_on) {
        // sampled-slip mode: the optimal rollout draws a fresh slip per transit as well (mppi.py:202-214 with
        // traversability_model.py:65-69).  Draws and the (mean, std) window are staged by all threads first.
        const float *__restrict__ sg = p.slip_std + (size_t)b * p.map_stride;
        float *zol = red + kRedFloats + tail_group_floats(nblk, PS);                      // T + 4 draws
        float2 *win2 = reinterpret_cast<float2 *>((reinterpret_cast<uintptr_t>(zol + tail_draw_floats(T)) + 7) & ~(uintptr_t)7);
        if (p.zo) {
            for (int t = tid; t < T; t += NT) zol[t] = p.zo[(size_t)b * T + t];
        } else {
            for (int j = tid; 4 * j < T; j += NT) philox_slip_block(p.seed, p.tail_solve, (uint32_t)b, 0xffffffffu, (uint32_t)j, zol + 4 * j);
        }
        if (LDSWIN) {
            w = window_origin<GEO>(p, sx, sy);
            for (int e = tid; e < p.WN * p.WN; e += NT) {
                const int r = e / p.WN, c = e - r * p.WN;
                const size_t g = (size_t)min(w.wy0 + r, p.G - 1) * p.G + min(w.wx0 + c, p.G - 1);
                win2[e] = make_float2(map[g], sg[g]);
            }
        }
        __syncthreads();
        BN_STAMP(12);
        if (tid == 0) {
            float *Xs = xl;                              // staged in LDS, written out coalesced below
            float xn, yn, tn;
            if (LDSWIN) {
                SlipChain c;
                c.x = sx; c.y = sy; c.th = sth;
                sincos_spec(c.th, c.sn, c.cs);
                c.e = slip_cell_safe<GEO, true>(p, w, sx, sy);
                slip_chain_step<GEO, true, REF>(p, win2, w, c, us[0], us[1], zol[0], xn, yn, tn);
                Xs[0] = xn; Xs[1] = yn; Xs[2] = tn;
                int t = 1;
                for (; t + 4 <= T; t += 4) {                 // controls and draws of four steps read up front
                    float uq[4][3];
#pragma unroll
                    for (int i = 0; i < 4; ++i) { uq[i][0] = us[2 * (t + i)]; uq[i][1] = us[2 * (t + i) + 1]; uq[i][2] = zol[t + i]; }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        slip_chain_step<GEO, false, REF>(p, win2, w, c, uq[i][0], uq[i][1], uq[i][2], xn, yn, tn);
                        Xs[3 * (t + i)] = xn; Xs[3 * (t + i) + 1] = yn; Xs[3 * (t + i) + 2] = tn;
                    }
                }
                for (; t < T; ++t) {
                    slip_chain_step<GEO, false, REF>(p, win2, w, c, us[2 * t], us[2 * t + 1], zol[t], xn, yn, tn);
                    Xs[3 * t] = xn; Xs[3 * t + 1] = yn; Xs[3 * t + 2] = tn;
                }
                Xs[3 * T] = c.x; Xs[3 * T + 1] = c.y; Xs[3 * T + 2] = c.th;
                BN_STAMP(11);
            } else {
                float x = sx, y = sy, th = sth;
                float sn, cs;
                sincos_spec(th, sn, cs);
                for (int t = 0; t < T; ++t) {
                    const int e = slip_cell_safe<GEO, false>(p, w, x, y);
                    const float trav = trav_from_slip(map[e], sg[e], zol[t]);
                    if constexpr (REF) {
                        sincos_spec(th, sn, cs);
                        const float tv = trav * us[2 * t];
                        xn = x + (tv * cs) * p.dt; yn = y + (tv * sn) * p.dt;
                        tn = th + (trav * us[2 * t + 1]) * p.dt;
                        th = wrap_angle(tn);
                    } else {
                    const float g = us[2 * t] * p.dt, dth = trav * (us[2 * t + 1] * p.dt);
                    xn = __builtin_fmaf(trav, g * cs, x); yn = __builtin_fmaf(trav, g * sn, y);
                    tn = theta_step(th, dth, t == 0);
                    rotate_spec(cs, sn, dth);
                    }
                    Xs[3 * t] = xn; Xs[3 * t + 1] = yn; Xs[3 * t + 2] = tn;
                    x = clampf(xn, p.x0, p.x_hi); y = clampf(yn, p.y0, p.y_hi);
                }
                Xs[3 * T] = x; Xs[3 * T + 1] = y; Xs[3 * T + 2] = th;
            }
        }
    }
    if (p.slip_on && tid < 64) {
        // wave 0: thread 0 ran the sampled chain above
    } else if (tid == 0) {
        // optimal_state_seq: batch-1 rollout of U* with the same aliasing (mppi.py:202-214)
        Chain c;
        c.x = sx; c.y = sy; c.th = sth;
        sincos_spec(c.th, c.sn, c.cs);
        c.trav = trav_lookup<GEO, LDSWIN, true>(p, win, map, w, c.x, c.y);
        float *Xs = xl;                              // staged in LDS, written out coalesced below
        float xn, yn, tn;
        if constexpr (REF) {
            chain_step<GEO, LDSWIN, true, true, false, 0, true>(p, win, map, w, c, us[0], us[1], xn, yn, tn);
            Xs[0] = xn; Xs[1] = yn; Xs[2] = tn;
            int t = 1;
            for (; t + 4 <= T; t += 4) {                   // controls of four steps read up front (LDS latency off the chain)
                float uq[4][2];
#pragma unroll
                for (int i = 0; i < 4; ++i) { uq[i][0] = us[2 * (t + i)]; uq[i][1] = us[2 * (t + i) + 1]; }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    chain_step<GEO, LDSWIN, false, true, false, 0, true>(p, win, map, w, c, uq[i][0], uq[i][1], xn, yn, tn);
                    Xs[3 * (t + i) + 0] = xn; Xs[3 * (t + i) + 1] = yn; Xs[3 * (t + i) + 2] = tn;
                }
            }
            for (; t < T; ++t) {
                chain_step<GEO, LDSWIN, false, true, false, 0, true>(p, win, map, w, c, us[2 * t], us[2 * t + 1], xn, yn, tn);
                Xs[3 * t + 0] = xn; Xs[3 * t + 1] = yn; Xs[3 * t + 2] = tn;
            }
        } else {
            // The chain form of the latency kernel (round 4): the next step's controls are folded into its factors at the end of each
            // step, under the gather's latency (PREP), and the window index is the three-instruction form (ASMIDX with the LDS window).
            // Same operations per step, so the same bits; this serial rollout is the last thing between a batch's final solve and
            // its results (4.5 -> ~3.8 us at T = 50), and part of every synchronous forward().
            constexpr int AI = LDSWIN ? 1 : 0;
            chain_prepare(p, c, us[0], us[1]);
            chain_step<GEO, LDSWIN, true, true, true, AI>(p, win, map, w, c, us[0], us[1], xn, yn, tn, T > 1 ? us[2] : 0.0f, T > 1 ? us[3] : 0.0f);
            Xs[0] = xn; Xs[1] = yn; Xs[2] = tn;
            int t = 1;
            for (; t + 4 <= T; t += 4) {                   // controls of four steps (and the first of the next four) read up front
                float uq[5][2];
#pragma unroll
                for (int i = 0; i < 5; ++i) { const int tt = min(t + i, T - 1); uq[i][0] = us[2 * tt]; uq[i][1] = us[2 * tt + 1]; }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    chain_step<GEO, LDSWIN, false, true, true, AI>(p, win, map, w, c, uq[i][0], uq[i][1], xn, yn, tn, uq[i + 1][0], uq[i + 1][1]);
                    Xs[3 * (t + i) + 0] = xn; Xs[3 * (t + i) + 1] = yn; Xs[3 * (t + i) + 2] = tn;
                }
            }
            for (; t < T; ++t) {
                const int tt = min(t + 1, T - 1);
                chain_step<GEO, LDSWIN, false, true, true, AI>(p, win, map, w, c, us[2 * t], us[2 * t + 1], xn, yn, tn, us[2 * tt], us[2 * tt + 1]);
                Xs[3 * t + 0] = xn; Xs[3 * t + 1] = yn; Xs[3 * t + 2] = tn;
            }
        }
        Xs[3 * T + 0] = c.x; Xs[3 * T + 1] = c.y; Xs[3 * T + 2] = c.th;
        BN_STAMP(11);
    } else if (NT > 64 && tid >= 64) {
        if (defer_tail_wait) {                         // every writing wave waits for itself: wave 0 is on the serial rollout, no barrier to meet at
            if ((tid & 63) == 0) {
                // (granule-polling self tail: the rows are here, the per-rollout costs -- plain device-scope stores -- only once every
                // rollout workgroup has counted itself in behind its acknowledged stores)
                if (self_gran) wait_counter(flag_ctr(p.flag_part, p.prev_slot * p.B + b), p.wait_part, p);
                wait_counter(flag_ctr(p.flag_tail, b), p.wait_tail, p);
            }
            store_ustar(tid - 64, NT - 64, tid == 64);
        }
        tail_weights<AGENT>(p, b, cost_all, K, m, S, tid, 64, NT - 64);
    }
    if constexpr (NT == 64) {                          // single-wave tail: the weights follow the X* rollout
        const float *cost = cost_all + (size_t)b * K;
        float *wout = p.w + (size_t)b * K;
        float *cout = p.cost_out + (size_t)b * K;
        for (int k = tid; k < K; k += 64) {
            const float ck = cost[k];
            cout[k] = ck;
            wout[k] = expf((-ck) / p.lambda_ - m) / S;
        }
    }
    // optimal_state_seq out of LDS: coalesced, and to the caller's copy of the packed U* | X* block as well
    BN_SSTAMP(4);
    __syncthreads();
    BN_SSTAMP(5);
    {
        float *Xg = p.xstar + (size_t)b * (T + 1) * 3;
        float *Xc = p.out_copy ? p.out_copy + (size_t)p.B * 2 * T + (size_t)b * (T + 1) * 3 : nullptr;
        for (int i = tid; i < 3 * (T + 1); i += NT) {
            const float v = xl[i];
            st<AGENT>(Xg + i, v);
            if (Xc) st<AGENT>(Xc + i, v);
        }
    }
    // one more tail done (counted per instance): what an overlapped successor's tail waits for before it takes the output buffers
    if (p.flag_tail) publish_counter(flag_ctr(p.flag_tail, b), tid);
    BN_SSTAMP(6);
}

}  // namespace

}  // namespace bn
