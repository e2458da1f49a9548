// rollout_role.inc -- the five-wave role-split rollout kernel and its launcher for ONE noise source (BN_ROLE_EPS);
// included by rollout_role_{philox,kt2,t2k}.hip so the three families compile in parallel.
#include "mppi_device.h"

// BN_ROLE_REF (rollout_role_ref_*.hip): the same kernels in the reference's operation order (BN_FLAG_REFERENCE_ORDER,
// chain_step<.., REF = true>: sincos_spec of every step's heading, x + ((trav v) cos) dt).  The chain wave then integrates and wraps
// the heading itself -- sin / cos of step t need theta_t -- and hands the un-wrapped theta~ of the slot on through the ring's .z,
// where the default arithmetic hands on the increment for consumer A to integrate.
#ifndef BN_ROLE_REF
#define BN_ROLE_REF false
#endif

namespace bn {

namespace {

// ------------------------------------------------------------------------------
// Rollout + cost kernel.  grid = rollout_grid (ceil(K/64) workgroups per instance, then the aux workgroups), block = 320 = 5
// wavefronts that all map lane -> rollout k = 64*blk + lane and split the work of those 64 rollouts by ROLE,
// because one wavefront issues one instruction every ~5 cycles whether or not it depends on the
// previous one (measured, tools/ubench2.hip: no intra-wave overlap) and the T-step recurrence is a
// serial instruction chain:
//   wave 0  chain      the recurrence only: transit + gather (chain_step), ~50 instructions/step
//   wave 1  producer   noise -> clamped controls for the first half of chunk c+2
//   wave 2  producer   ... second half of chunk c+2
//   wave 3  consumer A chunk c-1: trajectory stores, control cost (fp64 accumulation in step order)
//   wave 4  consumer B chunk c-1: stage cost (sqrt, collision flag; fp64 accumulation in step order)
// Chunks are TU = 4 steps; one LDS-only barrier per chunk hands the control tile forward and the
// chain's outputs (ring of 2 chunks) backward.  Each per-rollout sum is accumulated by one wave in
// step order, so the arithmetic is identical to a single sequential loop (Arithmetic spec).
// LDS: [ ring 2 x TU x 64 x float4 | final state + control-cost sum 5 x 64 | e 64 | window WN*WN | mean 2T | mean*inv_var 2T |
//        control tile 2T x 65 ]
// ------------------------------------------------------------------------------
template <int EPS, int GEO, bool LDSWIN, bool STORE_U, bool TICKET, bool REF>
__global__ __launch_bounds__(kRolloutThreads) void rollout_kernel(const SolveParams p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    BN_TRACE_BEGIN();
    const WgId wg = decode_wg(p);
    if (wg.idle) return;
    if (wg.aux) {
        // pipelined mode: the extra workgroup computes the tail of the PREVIOUS solve (U*, X*, weights)
        // while the other workgroups roll out this one.  In a launch that exceeds one resident round it starts late (in a slot
        // one of the first rollout workgroups freed) and holds a serial chain: it then runs at top priority so that it ends
        // before the rollouts do (64 instances of K=1024: 28.2 -> 27.4 us).  In a launch that fits one round the same
        // priority would take issue slots from the rollouts from the start (32 instances: 18.8 -> 21.4 us): not set there.
        if (p.aux_prio) __builtin_amdgcn_s_setprio(3);
        if (p.overlap) finish_body<GEO, LDSWIN, kRolloutThreads, false, true, false, REF>(p, wg.b, p.part_prev, p.cost_prev, p.state_prev, smem);
        else finish_body<GEO, LDSWIN, kRolloutThreads, false, false, false, REF>(p, wg.b, p.part_prev, p.cost_prev, p.state_prev, smem);
        BN_TRACE_END();
        return;
    }
    const int T = p.T, K = p.K;
    float *ring = smem;                               // first: 16-byte aligned for the b128 ring accesses
    float *fin = ring + 2 * TU * 4 * 64;
    float *el = fin + 5 * 64;
    float *win = el + 64;
    float *ml = win + (LDSWIN ? p.WN * p.WN : 0);
    float *mv = ml + 2 * T;
    float *Ul = mv + 2 * T;

    const int tid = threadIdx.x;
    const int wid = tid >> 6, lane = tid & 63;
    // A workgroup's waves are dealt to the 4 SIMDs cyclically, so waves 0 and 4 share one: they get the two
    // light consumer roles; the chain (role 0) has a SIMD to itself.  role: 0 chain, 1-2 producers, 3-4 consumers.
    const int wv = (wid == 0) ? 3 : (wid == 4) ? 4 : wid - 1;
    const int b = wg.b;
    const int k = wg.blk * kRolloutsPerBlock + lane;
    const bool active = k < K;
    const int kk = active ? k : K - 1;

    const float *__restrict__ map = p.map + (size_t)b * p.map_stride;
    const float *__restrict__ eps = p.eps;
    // open loop: the caller's state; closed loop: the previous solve's state, advanced below
    const float *st_src = p.closed_loop ? p.state_prev : p.state;
    float sx = st_src[b * 3 + 0], sy = st_src[b * 3 + 1], sth = st_src[b * 3 + 2];
    const float gx = p.goal[b * 2 + 0], gy = p.goal[b * 2 + 1];
    const uint64_t solve = p.solve;
    BN_STAMP(0);

    // warm start straight from the previous solve's per-block statistics (bit-identical to the U* the aux
    // block publishes): no kernel boundary between consecutive solves of one instance.  Its loads go out
    // first so that they and the window staging (which waits for the state) share one memory round trip.
    const float *part_prev = p.part_prev + (size_t)b * p.nblk * (2 + 2 * T);
    // Overlapped launch (p.overlap, open loop only): the previous solve of this instance may still be running in a launch on the
    // other stream.  The window goes first; then one lane waits for that solve's workgroups of THIS instance to have counted
    // themselves in (device counter), and the merge reads their rows with device-scope loads.  The workgroup holds its slot while
    // it waits: launches are dispatched instance by instance, so the instances a late launch waits for finish first.
    const bool ov = p.overlap && p.mean_from_part;
    MergeLoads pre{};
    const bool pre_ok = p.mean_from_part && p.nblk <= 64 && !ov;
    if (pre_ok) pre = merge_issue(part_prev, p.nblk, T, tid);

    Win w{0, 0, 0.f, 0.f, 0.f, 0.f};
    if (LDSWIN && !p.closed_loop) {
        w = window_origin<GEO>(p, sx, sy);
        stage_window(win, map, w, p.WN, p.G, tid, kRolloutThreads);
    }
    if (ov) {
        if (tid == 0) wait_counter<16>(flag_ctr(p.flag_part, p.prev_slot * p.B + b), p.wait_part, p);
        __syncthreads();
        if (p.closed_loop) {                           // the state the previous solve started from: published like its partials
            sx = load_agent(st_src + b * 3 + 0); sy = load_agent(st_src + b * 3 + 1); sth = load_agent(st_src + b * 3 + 2);
        }
        float m_unused, S_unused;
        merge_partials<kRolloutThreads, true>(part_prev, p.nblk, T, ml, ring, ring + p.nblk, tid, m_unused, S_unused, false, pre);
        for (int j = tid; j < 2 * T; j += kRolloutThreads) mv[j] = ml[j] * ((j & 1) ? p.iv1 : p.iv0);
    } else if (p.mean_from_part) {
        float m_unused, S_unused;
        merge_partials<kRolloutThreads>(part_prev, p.nblk, T, ml, ring, ring + p.nblk, tid, m_unused, S_unused, pre_ok, pre);
        for (int j = tid; j < 2 * T; j += kRolloutThreads) mv[j] = ml[j] * ((j & 1) ? p.iv1 : p.iv0);
    } else if (TICKET && p.overlap) {
        // Ticket path, overlapped launch (round 3): the previous solve -- a launch on the other stream, possibly still running --
        // merges its partials by ticket at its very end and counts that in (flag_part of its slot); the window above and this
        // workgroup's dispatch are already behind us when the merged mean arrives.  Device-scope loads: it was written by another kernel.
        if (tid == 0) wait_counter<16>(flag_ctr(p.flag_part, p.prev_slot * p.B + b), p.wait_part, p);
        __syncthreads();
        for (int j = tid; j < 2 * T; j += kRolloutThreads) {
            const float m = load_agent(p.mean + (size_t)b * 2 * T + j);
            ml[j] = m;
            mv[j] = m * ((j & 1) ? p.iv1 : p.iv0);
        }
    } else {
        for (int j = tid; j < 2 * T; j += kRolloutThreads) {
            const float m = p.mean[(size_t)b * 2 * T + j];
            ml[j] = m;
            mv[j] = m * ((j & 1) ? p.iv1 : p.iv0);      // mean[t] @ inv_cov (diagonal), mppi.py:179-180
        }
    }
    if (p.closed_loop) {
        // PlanetaryEnv.step with the previous solve's first control (ml[0..1] = U*_prev[0], published by the
        // barrier inside merge_partials): every workgroup advances the state itself, no launch in between
        const EnvStep e = env_advance<GEO>(p, b, sx, sy, sth, ml[0], ml[1], p.env_z, (uint64_t)p.ep_index);
        sx = e.x; sy = e.y; sth = e.th;
        if (LDSWIN) {
            w = window_origin<GEO>(p, sx, sy);
            stage_window(win, map, w, p.WN, p.G, tid, kRolloutThreads);
        }
    }
    const bool pub = !TICKET && p.flag_part != nullptr;   // member of an overlapped batch: what a successor reads goes out as device-scope stores
    const bool tpub = TICKET && p.flag_part != nullptr;   // ... on the ticket path: the costs (the next launch's aux workgroup reads them); the partials are device-scope anyway
    if (wg.blk == 0 && tid == 0) {                     // the state this solve starts from, for its tail and the next solve
        if (pub || (TICKET && p.flag_part != nullptr)) { store_agent(p.state_copy + b * 3 + 0, sx); store_agent(p.state_copy + b * 3 + 1, sy); store_agent(p.state_copy + b * 3 + 2, sth); }
        else { p.state_copy[b * 3 + 0] = sx; p.state_copy[b * 3 + 1] = sy; p.state_copy[b * 3 + 2] = sth; }
        if (p.state_snap) { p.state_snap[b * 3 + 0] = sx; p.state_snap[b * 3 + 1] = sy; p.state_snap[b * 3 + 2] = sth; }   // first launch of a journalled batch (SolveParams::state_snap)
    }
    BN_BAR();
    if (p.mean_snap && wg.blk == 0 && wid == 0) snapshot_mean(p, b, ml, lane);

    // Rows of X and U are pitched to Kp = 64 * nblk floats, so every lane stores unconditionally
    // (lanes past K write into the pad).
    const size_t Kp = (size_t)p.Kp;
    const bool lean = p.lean != 0;                    // lean mode: no trajectory batch (p.X is null)
    float *Xb = p.X + (size_t)b * (T + 1) * 3 * Kp + k;
    float *Ub = STORE_U ? p.U + (size_t)b * T * 2 * Kp + k : nullptr;

    // controls of chunks 0 and 1 (steps 0 .. 2*TU-1): TU/2 steps per wave (waves 0-3)
    if (wid < 4) {
#pragma unroll
        for (int q = 0; q < TU / 4; ++q) {
            const int t = wid * (TU / 2) + 2 * q;
            if (t < T) produce_pair<EPS, STORE_U>(p, eps, b, kk, t, solve, ml, Ul, Ub, Kp, lane);
        }
    }
    BN_BAR();
    BN_STAMP(1);

    Chain c;                                          // wave 0
    double Sd = 0.0, Ad = 0.0;                        // waves 4 / 3: fp64 accumulation of the fp32 terms (Arithmetic spec)
    float th_a = sth;                                 // wave 3: the heading as an output, integrated from the chain's increments
    if (wv == 0) {
        c.x = sx; c.y = sy; c.th = sth;               // mppi.py:160
        sincos_spec(c.th, c.sn, c.cs);
        c.trav = trav_lookup<GEO, LDSWIN, true>(p, win, map, w, c.x, c.y);
    }

    // wave 0: one chain step; emits what the reference leaves in slot t plus the traversability of state t+1.
    // The controls of the whole chunk are read from the LDS tile up front (uc[]): the compiler cannot hoist
    // those reads over the ring writes itself, and a 64-cycle LDS round trip per step would sit on the chain.
    // The ring writes come last (sched_barrier) so the wait for the gather overlaps the rest of the step.
#define BN_CHAIN(FIRST, i, slot)                                                                               \
    do {                                                                                                       \
        float xn, yn, dth;                              /* THETA = false: the heading increment comes back, theta stays with wave 3 */ \
        if constexpr (REF) chain_step<GEO, LDSWIN, FIRST, true, false, 0, true>(p, win, map, w, c, uc[i][0], uc[i][1], xn, yn, dth);   /* dth: theta~ of the slot */ \
        else chain_step<GEO, LDSWIN, FIRST, false, true>(p, win, map, w, c, uc[i][0], uc[i][1], xn, yn, dth,   \
                                                    i + 1 < TU ? uc[(i + 1) % TU][0] : un[0][0], i + 1 < TU ? uc[(i + 1) % TU][1] : un[0][1]);   \
        __builtin_amdgcn_sched_barrier(0);                                                                     \
        reinterpret_cast<float4 *>(slot)[lane] = make_float4(xn, yn, dth, c.trav);   /* one ds_write_b128 */    \
    } while (0)

    // wave 3: trajectory stores and control cost of one step
#define BN_CONSUME_A(t, o)                                                                                     \
    do {                                                                                                       \
        if (!lean) {                                                                                           \
        float *Xt = Xb + (size_t)(3 * (t)) * Kp;         /* slot t keeps the un-clamped state (aliasing) */     \
        Xt[0] = o.x; Xt[Kp] = o.y; Xt[2 * Kp] = REF ? o.z : theta_step(th_a, o.z, (t) == 0);   /* robot_model.py:88,90 */  \
        } else { asm volatile("" ::"v"(o.z)); }                                                                \
        const float u0 = Ul[(2 * (t)) * kUPad + lane], u1 = Ul[(2 * (t) + 1) * kUPad + lane];                  \
        const float a = mv[2 * (t)] * u0 + mv[2 * (t) + 1] * u1;            /* mppi.py:178-182 */             \
        Ad += (double)(p.lambda_ * a);                                                                         \
    } while (0)

    // wave 4: stage cost of one step.  The cell of the un-clamped slot equals the cell of the clamped
    // state (index clamp, grid_map.py:209), so the chain's gather serves stage cost t and transit t+1.
#define BN_CONSUME_B(t, o)                                                                                     \
    do {                                                                                                       \
        const float dx = o.x - gx, dy = o.y - gy;                                                              \
        const float sc = sqrt_cr_normal(dx * dx + dy * dy) + (o.w <= p.thr ? 1.0e4f : 0.0f);   /* objectives.py:47-53 */ \
        Sd += (double)sc;                                                                                      \
    } while (0)

    // One phase = one chunk of TU steps for the chain, the previous chunk for the consumer, the
    // chunk after next for the producers.  GUARD handles the ragged last chunk.
#define BN_PHASE(cc, FIRSTCHUNK, GUARD)                                                                        \
    do {                                                                                                       \
        if (wv == 0) {                                                                                         \
            if ((cc) * TU < T) {                                                                               \
                float *slot = ring + (((cc) & 1) * TU) * 256;                                                  \
                /* the NEXT chunk's controls (produced last phase, visible since the barrier) are read now and */ \
                /* land under this chunk's steps: no LDS round trip at the head of a phase                    */ \
                float un[TU][2];                                                                               \
                _Pragma("unroll") for (int i = 0; i < TU; ++i) {                                               \
                    const int t = min(((cc) + 1) * TU + i, T - 1);                                             \
                    un[i][0] = Ul[(2 * t) * kUPad + lane];                                                     \
                    un[i][1] = Ul[(2 * t + 1) * kUPad + lane];                                                 \
                }                                                                                              \
                __builtin_amdgcn_sched_barrier(0);                                                             \
                _Pragma("unroll") for (int i = 0; i < TU; ++i) {                                               \
                    const int t = (cc) * TU + i;                                                               \
                    if (!(GUARD) || t < T) {                                                                   \
                        if ((FIRSTCHUNK) && i == 0) BN_CHAIN(true, i, slot + i * 256);                         \
                        else BN_CHAIN(false, i, slot + i * 256);                                               \
                    }                                                                                          \
                }                                                                                              \
                _Pragma("unroll") for (int i = 0; i < TU; ++i) { uc[i][0] = un[i][0]; uc[i][1] = un[i][1]; }   \
            }                                                                                                  \
        } else if (wv >= 3) {                                                                                  \
            if ((cc) >= 1) {                                                                                   \
                const float *slot = ring + ((((cc) - 1) & 1) * TU) * 256;                                      \
                float4 rq[TU];                        /* the whole chunk in one burst of ds_read_b128 */      \
                _Pragma("unroll") for (int i = 0; i < TU; ++i)                                                 \
                    rq[i] = reinterpret_cast<const float4 *>(slot + i * 256)[lane];                            \
                _Pragma("unroll") for (int i = 0; i < TU; ++i) {                                               \
                    const int t = ((cc) - 1) * TU + i;                                                         \
                    if (!(GUARD) || t < T) {                                                                   \
                        if (wv == 3) BN_CONSUME_A(t, rq[i]);                                                   \
                        else BN_CONSUME_B(t, rq[i]);                                                           \
                    }                                                                                          \
                }                                                                                              \
            }                                                                                                  \
        } else {                                                                                               \
            _Pragma("unroll") for (int q = 0; q < TU / 4; ++q) {                                               \
                const int t = ((cc) + 2) * TU + (wv == 1 ? 0 : TU / 2) + 2 * q;                                \
                if (t < T) produce_pair<EPS, STORE_U>(p, eps, b, kk, t, solve, ml, Ul, Ub, Kp, lane);          \
            }                                                                                                  \
        }                                                                                                      \
    } while (0)

    const int nfull = T / TU;                         // chunks with all TU steps
    float uc[TU][2];                                  // chain: the controls of its current chunk
    if (wv == 0) {
#pragma unroll
        for (int i = 0; i < TU; ++i) {
            const int t = min(i, T - 1);
            uc[i][0] = Ul[(2 * t) * kUPad + lane];
            uc[i][1] = Ul[(2 * t + 1) * kUPad + lane];
        }
        if constexpr (!REF) chain_prepare(p, c, uc[0][0], uc[0][1]);
    }
    BN_PHASE(0, true, true);
    BN_BAR();
    BN_STAMP(2);
    int cc = 1;
    BN_TIMING_DO(
    unsigned long long busy = 0;
    )
    for (; cc < nfull; ++cc) {                        // steady state: chunks cc (chain) and cc-1 (consumer) are full
        BN_TIMING_DO(
        const unsigned long long t_a = __builtin_readcyclecounter();
        )
        BN_PHASE(cc, false, false);
        BN_TIMING_DO(
        busy += __builtin_readcyclecounter() - t_a;
        )
        BN_BAR();
    }
    BN_TIMING_DO(
    if (p.stamps && blockIdx.x == 0 && blockIdx.y == 0 && lane == 0) p.stamps[16 + wv] = busy;
    )
    for (; cc * TU < T + TU; ++cc) {                  // ragged tail and the consumer's drain
        BN_PHASE(cc, false, true);
        BN_BAR();
    }
#undef BN_PHASE
#undef BN_CONSUME_A
#undef BN_CONSUME_B
#undef BN_CHAIN
    BN_STAMP(3);

    if (wv == 0) {                                     // state T (clamped / wrapped) and its traversability
        fin[lane] = c.x; fin[64 + lane] = c.y; fin[192 + lane] = c.trav;
        if constexpr (REF) fin[128 + lane] = c.th;     // the wrapped heading of state T: the chain's own in the reference order
    } else if (wv == 3) {
        fin[256 + lane] = (float)Ad;                   // sum_t lambda * control cost, rounded once
    }
    BN_BAR();

    if (wv == 3) {
        if (!lean) {
            float *Xt = Xb + (size_t)(3 * T) * Kp;     // slot T: clamped / wrapped state (the heading: this wave's own)
            Xt[0] = fin[lane]; Xt[Kp] = fin[64 + lane]; Xt[2 * Kp] = REF ? fin[128 + lane] : th_a;
        }
    } else if (wv == 4) {
        const float xT = fin[lane], yT = fin[64 + lane], trT = fin[192 + lane], A = fin[256 + lane];
        const float dxT = xT - gx, dyT = yT - gy;
        const float term = sqrt_cr_normal(dxT * dxT + dyT * dyT) + (trT <= p.thr ? 1.0e4f : 0.0f);    // mppi.py:184
        const float cost = ((float)Sd + term) + A;                                             // mppi.py:186-190
        if (active) { if (pub || tpub) store_agent(p.cost + (size_t)b * K + k, cost); else p.cost[(size_t)b * K + k] = cost; }
        // block-local softmin statistics   mppi.py:193-199
        const float z = active ? (-cost) / p.lambda_ : -INFINITY;
        const float zmax = wave_max(z);
        const float e = active ? expf(z - zmax) : 0.0f;
        const float esum = wave_sum(e);
        el[lane] = e;
        if (lane == 0) {
            float *part = p.part + ((size_t)b * p.nblk + wg.blk) * (2 + 2 * T);
            if (TICKET || pub) { store_agent(part, zmax); store_agent(part + 1, esum); }
            else { part[0] = zmax; part[1] = esum; }
        }
    }
    BN_BAR();
    BN_STAMP(4);
    // weighted control sums of this block (column_sums: four lanes per column of the tile)
    if (!TICKET && pub) {
        column_sums<kRolloutThreads, true>(Ul, el, T, tid, p.part + ((size_t)b * p.nblk + wg.blk) * (2 + 2 * T));
        publish_counter(flag_ctr(p.flag_part, p.cur_slot * p.B + b), tid);      // every store above acknowledged, then the count
    } else {
        column_sums<kRolloutThreads, TICKET>(Ul, el, T, tid, p.part + ((size_t)b * p.nblk + wg.blk) * (2 + 2 * T));
    }
    BN_STAMP(5);
    // sizes the pipelined prologue merge does not take (K > 2048): the last workgroup merges, the tail rides in the next launch
    if (TICKET) ticket_merge<kRolloutThreads>(p, b, wg.blk, smem);
    BN_TRACE_END();
}

template <int EPS, int GEO, bool LDSWIN, bool STORE_U>
hipError_t launch_rollout_u(const SolveParams &p, hipStream_t s)
{
    const dim3 grid = rollout_grid(p, p.have_prev != 0);
    const size_t lds = rollout_lds_bytes(p);
    if (p.ticket) {
        hipError_t e = ensure_lds(rollout_kernel<EPS, GEO, LDSWIN, STORE_U, true, BN_ROLE_REF>, lds);
        if (e != hipSuccess) return e;
        rollout_kernel<EPS, GEO, LDSWIN, STORE_U, true, BN_ROLE_REF><<<grid, dim3(kRolloutThreads), lds, s>>>(p);
    } else {
        hipError_t e = ensure_lds(rollout_kernel<EPS, GEO, LDSWIN, STORE_U, false, BN_ROLE_REF>, lds);
        if (e != hipSuccess) return e;
        rollout_kernel<EPS, GEO, LDSWIN, STORE_U, false, BN_ROLE_REF><<<grid, dim3(kRolloutThreads), lds, s>>>(p);
    }
    return hipGetLastError();
}

template <int EPS, int GEO, bool LDSWIN>
hipError_t launch_rollout_t(const SolveParams &p, hipStream_t s)
{
    return p.U ? launch_rollout_u<EPS, GEO, LDSWIN, true>(p, s) : launch_rollout_u<EPS, GEO, LDSWIN, false>(p, s);
}

template <int EPS>
hipError_t launch_rollout_e(const SolveParams &p, hipStream_t s)
{
    const bool win = p.WN > 0;
    switch (geo_of(p)) {
    case kGeoPow2Origin0: return win ? launch_rollout_t<EPS, kGeoPow2Origin0, true>(p, s) : launch_rollout_t<EPS, kGeoPow2Origin0, false>(p, s);
    case kGeoPow2: return win ? launch_rollout_t<EPS, kGeoPow2, true>(p, s) : launch_rollout_t<EPS, kGeoPow2, false>(p, s);
    default: return win ? launch_rollout_t<EPS, kGeoGeneral, true>(p, s) : launch_rollout_t<EPS, kGeoGeneral, false>(p, s);
    }
}


}  // namespace

}  // namespace bn

#include "rollout_lat.inc"

namespace bn {

hipError_t BN_ROLE_LAUNCHER(const SolveParams &p, hipStream_t s)
{
    if (p.lat_kernel) return launch_lat_e<BN_ROLE_EPS>(p, s);
    return launch_rollout_e<BN_ROLE_EPS>(p, s);
}

#ifdef BN_ROLE_OCCUPANCY
int rollout_blocks_per_cu(const SolveParams &p)
{
    int n = 0;
    const size_t lds = rollout_lds_bytes(p);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, rollout_kernel<kEpsPhilox, kGeoPow2Origin0, true, false, false, false>, kRolloutThreads, lds) != hipSuccess) return -1;
    return n;
}

#endif

}  // namespace bn
