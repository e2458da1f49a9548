// mppi_merge.h -- the workgroup's weighted control sums and the softmin merges of the per-workgroup partials: in a tail, in a
// rollout workgroup's prologue, by ticket.
#pragma once
#include "mppi_sync.h"
#include "mppi_stamps.h"
#include <math.h>

namespace bn {

namespace {

// First launch of the batches enqueued since the host last checked the error word: workgroup 0 of every instance keeps the mean
// this solve samples around (ml, in LDS), so that the host can re-run those batches on one stream should a wait expire.
__device__ __forceinline__ void snapshot_mean(const SolveParams &p, int b, const float *ml, int lane)
{
    for (int j = lane; j < 2 * p.T; j += 64) p.mean_snap[(size_t)b * 2 * p.T + j] = ml[j];
}

// The workgroup's weighted control sums  sum_k e_k u_k[j]  (mppi.py:196-199, before the cross-workgroup merge) for the
// 2T columns j of the LDS control tile (pitch kUPad).  One definition of the summation order for every rollout kernel,
// so that all of them produce the same bits: the 64 rollouts in four quarters of 16, each summed in rollout order with
// fma, combined as (q0 + q1) + (q2 + q3).  Here four adjacent lanes take the quarters of one column (2T x 4 work items
// over NT threads; 64 sequential fma per column on a quarter of the threads was 0.55 us of a 13 us solve) and the
// combination is two DPP quad permutes.  NT and the item count are multiples of 4: a quad is active as a whole.
template <int NT, bool AGENT>
__device__ __forceinline__ void column_sums(const float *Ul, const float *el, int T, int tid, float *part,
                                            unsigned long long *grow = nullptr, uint32_t tag = 0)
{
    for (int it = tid; it < 8 * T; it += NT) {
        const int j = it >> 2, r = it & 3;
        const float *col = Ul + j * kUPad + 16 * r, *e = el + 16 * r;
        float acc = 0.0f;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc = __builtin_fmaf(e[q], col[q], acc);
        asm volatile("s_nop 1\n\t"
                     "v_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
                     "v_add_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\ts_nop 1"
                     : "+v"(acc));
        if (r == 0) {
            if (grow) store_granule(grow + 2 + j, acc, tag);           // first: what the successor's prologue polls
            if (AGENT) store_agent(part + 2 + j, acc); else part[2 + j] = acc;
        }
    }
}

// ------------------------------------------------------------------------------
// Softmin merge and the tail of a solve (shared by the finish kernel, the aux block of the
// pipelined rollout kernel, and the rollout blocks' own prologue merge).
// ------------------------------------------------------------------------------
template <int NT>
__device__ __forceinline__ float block_reduce(float v, float *red, int tid, bool is_max)
{
    v = is_max ? wave_max(v) : wave_sum(v);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    float r = red[0];
    for (int i = 1; i < NT / 64; ++i) r = is_max ? fmaxf(r, red[i]) : r + red[i];
    __syncthreads();
    return r;
}

// Merge the nblk per-block statistics (max z, sum e, sum e*u) of one instance into
//   U*[j] = sum_k w_k u_k[j]      mppi.py:193-199
// written to us[0..2T) (LDS).  Deterministic: every caller (any thread count NT) gets bit-identical values,
// which is what lets each rollout block of the next solve recompute the warm-start mean on its own.
// LDS scratch: sc[nblk], red[4].  Returns (max z, sum exp) for the weights.
constexpr int kRedFloats = 32;      // red[]: block_reduce's per-wave values (at most 16), 32 floats wherever a merge's LDS is laid out
constexpr int kMergePrefetch = 16;
struct MergeLoads { float v[kMergePrefetch]; float mi, si; int j; };

// Which column of U* a thread of an NT-thread workgroup merges: its own index, rotated by c0 threads.  The latency kernel gives the
// columns to the waves that have a SIMD to themselves (c0 = 128: waves 2 and 3 take 2T <= 128 columns; waves 0 and 4 share a SIMD and
// were the last to reach the barrier behind the merge by 0.5 us, tools/stamps_overlap.py).  Who merges a column does not change its bits.
template <int NT>
__device__ __forceinline__ int merge_column(int tid, int c0) { return tid >= c0 ? tid - c0 : tid + NT - c0; }

// Issue every load of the few-blocks merge (nblk <= 64) without consuming any: lets the caller put
// other memory traffic (the window staging) in flight underneath.
template <bool AGENT = false>
__device__ __forceinline__ MergeLoads merge_issue(const float *__restrict__ part, int nblk, int T, int tid)
{
#define BN_PLD(ix) (AGENT ? load_agent(part + (ix)) : part[(ix)])
    const int PS = 2 + 2 * T;
    const int lane = tid & 63;
    MergeLoads L;
    L.j = tid < 2 * T ? tid : 0;
#pragma unroll
    for (int i = 0; i < kMergePrefetch; ++i) L.v[i] = BN_PLD((size_t)min(i, nblk - 1) * PS + 2 + L.j);
    const bool has = lane < nblk;
    L.mi = has ? BN_PLD((size_t)lane * PS) : -INFINITY;
    L.si = has ? BN_PLD((size_t)lane * PS + 1) : 0.0f;
    return L;
#undef BN_PLD
}

// The same loads from the granule copy of the rows (nblk <= kMergePrefetch), each checked against the producing solve's tag:
// `ok` stays true only if every granule this thread needs carried it.
// `col`: the column this thread merges (merge_column: not necessarily its thread index).
__device__ __forceinline__ MergeLoads merge_issue_granules(const unsigned long long *__restrict__ grows, int nblk, int T, int tid, uint32_t tag, bool &ok, int col)
{
    const int PS = 2 + 2 * T;
    const int lane = tid & 63;
    MergeLoads L;
    L.j = col < 2 * T ? col : 0;
    ok = true;
#pragma unroll
    for (int i = 0; i < kMergePrefetch; ++i) L.v[i] = load_granule(grows + (size_t)min(i, nblk - 1) * PS + 2 + L.j, tag, ok);
    const bool has = lane < nblk;
    bool ok2 = true;
    const float mi = load_granule(grows + (size_t)min(lane, nblk - 1) * PS, tag, ok2);
    const float si = load_granule(grows + (size_t)min(lane, nblk - 1) * PS + 1, tag, ok2);
    ok = ok && ok2;
    L.mi = has ? mi : -INFINITY;
    L.si = has ? si : 0.0f;
    return L;
}

// Split-phase form of merge_issue_granules: issue() puts the 18 loads of one poll on the wire, take() looks at them (the compiler's
// vmcnt wait lands there, not at the issue).
struct GranulePoll {
    unsigned long long v[kMergePrefetch], mi, si;
    __device__ __forceinline__ void issue(const unsigned long long *__restrict__ grows, int nblk, int T, int lane, int col)
    {
        const int PS = 2 + 2 * T;
        const int j = col < 2 * T ? col : 0;
#pragma unroll
        for (int i = 0; i < kMergePrefetch; ++i)
            v[i] = __hip_atomic_load(grows + (size_t)min(i, nblk - 1) * PS + 2 + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        mi = __hip_atomic_load(grows + (size_t)min(lane, nblk - 1) * PS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        si = __hip_atomic_load(grows + (size_t)min(lane, nblk - 1) * PS + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // all of this lane's granules carry `tag`?  L: the values, laid out as merge_issue_granules leaves them
    __device__ __forceinline__ bool take(uint32_t tag, int nblk, int T, int lane, int col, MergeLoads &L) const
    {
        bool ok = (uint32_t)(mi >> 32) == tag && (uint32_t)(si >> 32) == tag;
#pragma unroll
        for (int i = 0; i < kMergePrefetch; ++i) { ok = ok && (uint32_t)(v[i] >> 32) == tag; L.v[i] = __uint_as_float((uint32_t)v[i]); }
        const bool has = lane < nblk;
        L.mi = has ? __uint_as_float((uint32_t)mi) : -INFINITY;
        L.si = has ? __uint_as_float((uint32_t)si) : 0.0f;
        L.j = col < 2 * T ? col : 0;
        return ok;
    }
};

// U*[column L.j] from one thread's prefetched rows (nblk <= kMergePrefetch): the arithmetic of merge_partials' few-blocks branch,
// operation for operation, for a caller that wants the value in a register instead of in LDS.  Every lane of the wave must call it.
__device__ __forceinline__ float merge_one(const MergeLoads &L, int nblk, int lane)
{
    const float m = wave_max(L.mi);
    const float f = lane < nblk ? expf(L.mi - m) : 0.0f;
    const float S = wave_sum(L.si * f);
    const int fb = __float_as_int(f);
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < kMergePrefetch; ++i) acc = __builtin_fmaf(L.v[i], __int_as_float(__builtin_amdgcn_readlane(fb, i)), acc);   // f == 0 past nblk
    return acc / S;
}

// Two-level merge for more than 64 partial rows (K > 4096): rows are first merged in groups of kGroupRows
// consecutive rows, each relative to its group's max -- by whichever wave(s) get the job: a wave of the stand-alone
// tail, or the waves of the last rollout workgroup of the group to finish (ticket) -- then the group rows are merged
// like ordinary partials.  One definition for every caller, so the result does not depend on who ran it.
constexpr int kGroupRows = 16;

// Rows [row0, row0 + nrows) of `part` -> one row `gout` = (group max, sum e, sum e*u[2T]).  One wave; it handles the
// 64-column blocks cb0, cb0 + cbstep, ... (several waves may share a group: they derive identical scales).
template <bool AGENT, bool AGENT_STORE>
__device__ __forceinline__ void merge_group(const float *__restrict__ part, int row0, int nrows, int T, int lane, int cb0,
                                            int cbstep, float *gout)
{
#define BN_PLD(ix) (AGENT ? load_agent(part + (ix)) : part[(ix)])
#define BN_PST(ptr, val) do { if (AGENT_STORE) store_agent((ptr), (val)); else *(ptr) = (val); } while (0)
    const int PS = 2 + 2 * T;
    const bool has = lane < nrows;
    const float mi = has ? BN_PLD((size_t)(row0 + lane) * PS) : -INFINITY;
    const float si = has ? BN_PLD((size_t)(row0 + lane) * PS + 1) : 0.0f;
    float v[kGroupRows];
    int jj = lane + 64 * cb0;
#pragma unroll
    for (int r = 0; r < kGroupRows; ++r) v[r] = (r < nrows && jj < 2 * T) ? BN_PLD((size_t)(row0 + r) * PS + 2 + jj) : 0.0f;
    const float mg = wave_max(mi);
    const float f = has ? expf(mi - mg) : 0.0f;
    const float sg = wave_sum(si * f);
    const int fb = __float_as_int(f);
    for (int cb = cb0;;) {
        float acc = 0.0f;
#pragma unroll
        for (int r = 0; r < kGroupRows; ++r) acc = __builtin_fmaf(v[r], __int_as_float(__builtin_amdgcn_readlane(fb, r)), acc);   // f == 0 past nrows
        if (jj < 2 * T) BN_PST(gout + 2 + jj, acc);
        cb += cbstep;
        if (64 * cb >= 2 * T) break;
        jj = lane + 64 * cb;
#pragma unroll
        for (int r = 0; r < kGroupRows; ++r) v[r] = (r < nrows && jj < 2 * T) ? BN_PLD((size_t)(row0 + r) * PS + 2 + jj) : 0.0f;
    }
    if (cb0 == 0 && lane == 0) { BN_PST(gout, mg); BN_PST(gout + 1, sg); }
#undef BN_PLD
#undef BN_PST
}

// BIG = false leaves the two-level code out of callers that never see more than 64 rows (the rollout kernels'
// prologue / aux / ticket merges): it costs them registers.
// SYNC = false leaves out the closing barrier: for a caller whose threads go on to use only the us[] entries they wrote
// themselves (jj = tid, tid + NT, ...) and that has a barrier of its own before anybody reads somebody else's.
// WIDE picks how the rows beyond the prefetched 16 are loaded (same arithmetic either way): sixteen at a time through a second
// register array (kernels that own a CU: the latency kernel, the stand-alone tail), or eight at a time from one address register
// (the role and one-wave kernels, whose occupancy hangs on ~80 VGPRs and no scratch segment: tests/test_build_artifacts.py).
template <int NT, bool AGENT = false, bool BIG = false, bool SYNC = true, bool WIDE = false>
__device__ __forceinline__ void merge_partials(const float *__restrict__ part, int nblk, int T, float *us, float *sc,
                                               float *red, int tid, float &m_out, float &S_out, bool have_pre, const MergeLoads &pre,
                                               int c0 = 0)
{
    const int col = merge_column<NT>(tid, c0);
#define BN_PLD(ix) (AGENT ? load_agent(part + (ix)) : part[(ix)])
    const int PS = 2 + 2 * T;
    const int lane = tid & 63;
    float m, S;
    if (nblk <= 64) {
        // Few blocks (K <= 4096): every wave reduces the nblk (max, sum) pairs itself -- same inputs,
        // same operations, so all waves (and all workgroups) hold identical m, S and scales -- and all
        // loads are issued before the first use: one memory round trip, one barrier.
        const MergeLoads L = have_pre ? pre : merge_issue<AGENT>(part, nblk, T, tid);
        m = wave_max(L.mi);
        const float f = lane < nblk ? expf(L.mi - m) : 0.0f;       // scale of block `lane`; 0 past nblk
        S = wave_sum(L.si * f);
        // scale of block i = lane i's f, read with v_readlane (ignores EXEC): only the lanes with jj < 2T enter the
        // loop below, and a ds_bpermute shuffle returns nothing from the lanes that did not
        const int fb = __float_as_int(f);
#define BN_SCALE(i) __int_as_float(__builtin_amdgcn_readlane(fb, (i)))
        for (int jj = col; jj < 2 * T; jj += NT) {
            float acc = 0.0f;
            int i0 = 0;
            if (jj == L.j) {
#pragma unroll
                for (int i = 0; i < kMergePrefetch; ++i) acc = __builtin_fmaf(L.v[i], BN_SCALE(i), acc);   // f == 0 past nblk
                i0 = kMergePrefetch;
            }
            // Rows beyond the prefetched ones with several loads in flight (one at a time, each behind the previous row's FMA, 48
            // device-scope loads cost a K=4096 solve 13 us).  A second 16-entry array costs the role kernel 25 VGPRs, reusing the
            // prefetch array a scratch segment, eight scalars with 64-bit addresses 8 VGPRs too many -- each 17-35 % of its
            // throughput at four workgroups per CU (tools/config_rate.py) --, hence the two forms.
            if constexpr (WIDE) {
                for (; i0 < nblk; i0 += kMergePrefetch) {
                    float v[kMergePrefetch];
#pragma unroll
                    for (int q = 0; q < kMergePrefetch; ++q) v[q] = BN_PLD((size_t)min(i0 + q, nblk - 1) * PS + 2 + jj);
#pragma unroll
                    for (int q = 0; q < kMergePrefetch; ++q)
                        if (i0 + q < nblk) acc = __builtin_fmaf(v[q], BN_SCALE(i0 + q), acc);
                }
            } else {
                for (; i0 < nblk; i0 += 8) {
                    // one 32-bit offset from the (uniform) row base, the eight rows at constant distances: one address register
                    const float *row = part + (unsigned)(i0 * PS + 2 + jj);
                    const int left = nblk - i0;
                    float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f, v4 = 0.f, v5 = 0.f, v6 = 0.f, v7 = 0.f;
    #define BN_ROW(k) (AGENT ? load_agent(row + (k) * PS) : row[(k) * PS])
                    v0 = BN_ROW(0);
                    if (left > 1) v1 = BN_ROW(1);
                    if (left > 2) v2 = BN_ROW(2);
                    if (left > 3) v3 = BN_ROW(3);
                    if (left > 4) v4 = BN_ROW(4);
                    if (left > 5) v5 = BN_ROW(5);
                    if (left > 6) v6 = BN_ROW(6);
                    if (left > 7) v7 = BN_ROW(7);
    #undef BN_ROW
                    acc = __builtin_fmaf(v0, BN_SCALE(i0), acc);
                    if (left > 1) acc = __builtin_fmaf(v1, BN_SCALE(i0 + 1), acc);
                    if (left > 2) acc = __builtin_fmaf(v2, BN_SCALE(i0 + 2), acc);
                    if (left > 3) acc = __builtin_fmaf(v3, BN_SCALE(i0 + 3), acc);
                    if (left > 4) acc = __builtin_fmaf(v4, BN_SCALE(i0 + 4), acc);
                    if (left > 5) acc = __builtin_fmaf(v5, BN_SCALE(i0 + 5), acc);
                    if (left > 6) acc = __builtin_fmaf(v6, BN_SCALE(i0 + 6), acc);
                    if (left > 7) acc = __builtin_fmaf(v7, BN_SCALE(i0 + 7), acc);
                }
            }
            us[jj] = acc / S;
        }
#undef BN_SCALE
    } else if (BIG && nblk <= 64 * kGroupRows) {
        // two-level (see merge_group): groups dealt to the waves, group rows in LDS, then the few-rows merge above
        constexpr int NW = NT / 64;
        const int ng = (nblk + kGroupRows - 1) / kGroupRows;
        float *grows = red + kRedFloats;                         // ng x PS
        for (int g = tid >> 6; g < ng; g += NW)
            if constexpr (BIG) merge_group<AGENT, false>(part, g * kGroupRows, min(kGroupRows, nblk - g * kGroupRows), T, lane, 0, 1, grows + (size_t)g * PS);
        __syncthreads();
        merge_partials<NT, false, false>(grows, ng, T, us, sc, red, tid, m, S, false, MergeLoads{});
        m_out = m;
        S_out = S;
        return;
    } else {
        // more than 1024 workgroups (K > 65536): plain column sums in row order (independent of NT as well)
        float mm = -INFINITY;
        for (int i = tid; i < nblk; i += NT) mm = fmaxf(mm, BN_PLD((size_t)i * PS));
        m = block_reduce<NT>(mm, red, tid, true);
        float s = 0.0f;
        for (int i = tid; i < nblk; i += NT) {
            const float f = expf(BN_PLD((size_t)i * PS) - m);
            sc[i] = f;
            s += BN_PLD((size_t)i * PS + 1) * f;
        }
        S = block_reduce<NT>(s, red, tid, false);        // the barrier inside also publishes sc[]
        for (int jj = tid; jj < 2 * T; jj += NT) {
            float acc = 0.0f;
            for (int i = 0; i < nblk; ++i) acc = __builtin_fmaf(BN_PLD((size_t)i * PS + 2 + jj), sc[i], acc);
            us[jj] = acc / S;
        }
    }
    if (SYNC) __syncthreads();
    m_out = m;
    S_out = S;
#undef BN_PLD
}

// Ticket merge: every workgroup of instance b publishes its partials, takes a ticket, and the one that draws the
// last ticket merges all of them (fixed order: the result does not depend on which workgroup that is) into
// U* = the next mean, plus the softmin statistics the tail needs for the weights.  Saves the merge launch.
// With more than 64 workgroups the merge is the two-level one (merge_group): the last workgroup of each group of 16
// merges its group (its waves split the columns: one memory round trip), the last group to finish merges the groups.
// The partials travel as device-scope sc1 stores / loads (store_agent / load_agent): once every wave has seen its
// stores acknowledged (vmcnt 0) and the workgroup has met at the barrier, the ticket is taken.  No __threadfence:
// that writes back / invalidates the whole L2 once per workgroup (measured: +18 us per launch at 128 workgroups).
// Ticket counters: kTicketStride ints per instance, [0] = groups (or workgroups) done, [1 + g] = workgroups of group g.
// LDS scratch: [ us 2T | sc nblk | red 32 | flag ].  Needs nblk <= 1024 (two levels).
constexpr int kTicketStride = 1 + 64;

template <int NT>
__device__ __forceinline__ void ticket_merge(const SolveParams &p, int b, int blk, float *scratch)
{
    const int T = p.T, tid = threadIdx.x, PS = 2 + 2 * p.T;
    float *us = scratch, *sc = us + 2 * T, *red = sc + p.nblk;
    int *flag = reinterpret_cast<int *>(red + kRedFloats);       // at most 64 rows reach merge_partials here: no group rows in LDS
    int *ticket = p.ticket + (size_t)b * kTicketStride;
    const float *part = p.part + (size_t)b * p.nblk * PS;
    const float *rows = part;
    int nrows = p.nblk;
    if (p.nblk > 64) {
        const int g = blk / kGroupRows, ng = (p.nblk + kGroupRows - 1) / kGroupRows;
        const int in_group = min(kGroupRows, p.nblk - g * kGroupRows);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) *flag = (atomicAdd(ticket + 1 + g, 1) == in_group - 1) ? 1 : 0;
        __syncthreads();
        if (!*flag) return;
        if (tid == 0) __hip_atomic_store(ticket + 1 + g, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (an overlapped successor takes its tickets behind the count below)
        float *grow = p.gpart + ((size_t)b * 64 + g) * PS;
        merge_group<true, true>(part, g * kGroupRows, in_group, T, tid & 63, tid >> 6, NT / 64, grow);
        rows = p.gpart + (size_t)b * 64 * PS;
        nrows = ng;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) *flag = (atomicAdd(ticket, 1) == nrows - 1) ? 1 : 0;
    __syncthreads();
    if (!*flag) return;
    BN_STAMP_ANY(6);
    if (tid == 0) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch (ordered by the stream, or by the count below)
    float m, S;
    merge_partials<NT, true, false>(rows, nrows, T, us, sc, red, tid, m, S, false, MergeLoads{});
    // Member of an overlapped batch (p.flag_part): the next launch may be running already -- on the other stream, its workgroups
    // waiting for exactly this -- so what it reads goes out as device-scope stores and the merge counts itself in behind them.
    const bool pubm = p.flag_part != nullptr;
    const bool spoiled = pubm && batch_spoiled(p);         // (see raise_wait_expired)
    for (int j = tid; j < 2 * T; j += NT) {
        const size_t at = (size_t)b * 2 * T + j;
        if (pubm) {
            store_agent(p.ustar_cur + at, us[j]);
            if (spoiled) continue;
            if (p.mean_used) store_agent(p.mean_used + at, load_agent(p.mean + at));
            store_agent(p.mean + at, us[j]);
        } else {
            p.ustar_cur[at] = us[j];
            if (p.mean_used) p.mean_used[at] = p.mean[at];   // what this solve sampled around
            p.mean[at] = us[j];                        // _previous_action_seq = U*, no shift (mppi.py:217)
        }
    }
    if (tid == 0) {
        if (pubm) { store_agent(p.stats_cur + b * 2 + 0, m); store_agent(p.stats_cur + b * 2 + 1, S); }
        else { p.stats_cur[b * 2 + 0] = m; p.stats_cur[b * 2 + 1] = S; }
    }
    if (pubm) publish_counter(flag_ctr(p.flag_part, p.cur_slot * p.B + b), tid);
    BN_STAMP_ANY(7);
}

}  // namespace

}  // namespace bn
