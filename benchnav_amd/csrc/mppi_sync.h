// mppi_sync.h -- wave reductions and what workgroups of one or several launches exchange data with: agent-scope loads and
// stores, counters, granules, the LDS-only barrier.
#pragma once
#include "mppi_kernels.h"

namespace bn {

namespace {

// Wave-wide reductions with DPP row shifts / row broadcasts: six VALU instructions instead of six ds_bpermute round trips
// through the LDS crossbar (~70 cycles each for a lone wave).  Written as inline assembly on purpose: expressed with
// __builtin_amdgcn_update_dpp, hipcc's DPP combiner mis-folded the update_dpp + add pairs inside the rollout kernel (wrong
// sums on hardware, correct in an isolated kernel).  The assembler adds no hazard padding inside an asm block, so the
// two wait states a DPP read needs after the VALU write of its source are spelled out (s_nop 1).
// Lanes whose DPP source does not exist are disabled (no bound_ctrl) and keep their accumulator.  After the six steps
// lane 63 holds the reduction of all 64 lanes; v_readlane hands it to everyone.  The order of the additions is fixed
// (inclusive scan within rows of 16, then across rows): every kernel and every caller gets the same bits.
#define BN_DPP_REDUCE(OP, v)                                                                                   \
    asm volatile("s_nop 1\n\t"                                                                                 \
                 OP " %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"                          \
                 OP " %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"                          \
                 OP " %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"                          \
                 OP " %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"                          \
                 OP " %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\ts_nop 1\n\t"                       \
                 OP " %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\ts_nop 1"                            \
                 : "+v"(v))

__device__ __forceinline__ float wave_max(float v)
{
    BN_DPP_REDUCE("v_max_f32_dpp", v);
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ float wave_sum(float v)
{
    BN_DPP_REDUCE("v_add_f32_dpp", v);
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// Device-scope accesses that bypass the per-XCD L2 (sc1): what lets workgroups on different XCDs exchange their
// partials inside one launch without a full L2 write-back / invalidate (see ticket_merge).
__device__ __forceinline__ void store_agent(float *ptr, float v) { __hip_atomic_store(ptr, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float load_agent(const float *ptr) { return __hip_atomic_load(ptr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <bool AGENT>
__device__ __forceinline__ float ld(const float *ptr) { return AGENT ? load_agent(ptr) : *ptr; }
template <bool AGENT>
__device__ __forceinline__ void st(float *ptr, float v) { if (AGENT) store_agent(ptr, v); else *ptr = v; }

// Overlapped launches: a counter another launch advances (device-scope atomics) reaches `need`.  ONE lane polls, with sc1 loads
// and s_sleep in between; the caller puts a workgroup barrier behind it.  Bounded: a wait that does not end within ~2 s sets
// *err and gives up -- a wrong result that the host sees at its next synchronising call (and repairs: recover_overlap in mppi_capi.cpp), never a hung GPU.
// SLEEP: s_sleep argument between polls (x 64 cycles).  1 where the wait is short and on the critical path (latency kernel); the
// role kernel's workgroups may hold a slot for many microseconds with hundreds of them polling at once -- at s_sleep 1 their
// loads saturate the memory channel the counters live in and everything else that touches it (measured: 40 instances, 31 us
// per launch instead of 21) -- so they poll every ~0.5 us, and the counters are kFlagStride apart (one channel each).
__device__ __forceinline__ unsigned long long *flag_ctr(unsigned long long *base, int i) { return base + (size_t)i * kFlagStride; }

// The error word lives in pinned host memory (SolveParams::err): a system-scope store, so that the host sees it without a copy.
// ... and in a device word (SolveParams::err_dev) that every later WRITER of the warm-start mean looks at first: a launch whose wait
// expired goes on with incomplete partials, and whatever is merged from them must not reach `mean` -- it is the one piece of state
// the re-run starts from (mean_snap is taken from it by the first launch of a stretch, which in exactly this situation may run
// LATE: round 4 saw NaN survive a repair that way).  The flag is raised before the workgroup publishes anything, so whoever sees
// its counts sees the flag.
__device__ __forceinline__ void raise_wait_expired(const SolveParams &p, const unsigned long long *ctr = nullptr, unsigned long long need = 0)
{
#ifdef BN_EXPERIMENTS                                  // which wait it was, for the host's message (tools/_repro*.py)
    if (__hip_atomic_load(p.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0) {
        p.err[8] = ctr ? (int)((ctr - p.flag_part) / kFlagStride) : -1; p.err[9] = (int)need;
        p.err[10] = ctr ? (int)__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : -1; p.err[11] = (int)p.solve;
        p.err[12] = blockIdx.x; p.err[13] = blockIdx.y; p.err[14] = p.have_prev * 100 + p.overlap * 10 + p.cur_slot; p.err[15] = (int)p.wait_part * 1000 + (int)p.wait_tail;
    }
#endif
    __hip_atomic_store(p.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (p.err_dev) __hip_atomic_store(p.err_dev, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ bool batch_spoiled(const SolveParams &p)
{
    return p.err_dev != nullptr && __hip_atomic_load(p.err_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
}

template <int SLEEP = 1>
__device__ __forceinline__ void wait_counter(const unsigned long long *ctr, unsigned long long need, const SolveParams &p)
{
    for (int it = 0; it < (1 << 23) / SLEEP + 1024; ++it) {
        if (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= need) return;
        __builtin_amdgcn_s_sleep(SLEEP);
    }
    raise_wait_expired(p, ctr, need);
}

// Publish: every wave has seen its own sc1 stores acknowledged (vmcnt 0), the workgroup meets, one lane counts it in.
__device__ __forceinline__ void publish_counter(unsigned long long *ctr, int tid)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) __hip_atomic_fetch_add(ctr, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Granules: an 8-byte {value, tag} pair written by ONE device-scope store, so a reader that sees the tag sees the value.
// The partial rows an overlapped successor's prologue needs are published this way as well (tag = producing solve's
// index + 1): it can poll the rows themselves -- one memory round trip -- instead of a counter and then the rows.
__device__ __forceinline__ void store_granule(unsigned long long *ptr, float v, uint32_t tag)
{
    __hip_atomic_store(ptr, ((unsigned long long)tag << 32) | (unsigned long long)__float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// ... to pinned host memory (system scope): what the host polls in bn_mppi_first_action
__device__ __forceinline__ void store_granule_host(unsigned long long *ptr, float v, uint32_t tag)
{
    __hip_atomic_store(ptr, ((unsigned long long)tag << 32) | (unsigned long long)__float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ float load_granule(const unsigned long long *ptr, uint32_t tag, bool &ok)
{
    const unsigned long long g = __hip_atomic_load(ptr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ok = ok && (uint32_t)(g >> 32) == tag;
    return __uint_as_float((uint32_t)g);
}

// Workgroup barrier that only drains LDS traffic: global stores of the consumer wave stay in flight.
#define BN_BAR() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

}  // namespace

}  // namespace bn
