// mppi_shard.cpp -- K-sharded solves of the C ABI: the rollouts of one shard, the caller-driven exchange
// (bn_mppi_shard_partials / bn_mppi_shard_finish_async) and the exchange the library enqueues itself through RCCL.
#include "mppi_handle.h"

#include <cstring>
#include <dlfcn.h>
#include <rccl/rccl.h>      // types only: the library itself is opened at run time (rccl_api), and only by a K-sharded solve

using namespace bn::host;

extern "C" {

int bn_mppi_set_rollout_offset(bn_mppi_t *h, int64_t first_rollout)
{
    if (!h) return fail(BN_ERR_INVALID, "null handle");
    if (first_rollout < 0 || first_rollout + h->p.K > 0x7fffffffLL) return fail(BN_ERR_INVALID, "first_rollout out of range");
    BN_BIND(h);
    if (int rc = settle_point(h)) return rc;
    if (int rc = flush_tail(h)) return rc;
    h->p.k0 = (int)first_rollout;
    return BN_OK;
}

int bn_mppi_shard_rollout_async(bn_mppi_t *h, const float *states, bn_mem_kind states_where, const float *eps,
                                bn_noise_kind noise)
{
    if (h && h->p.B != 1) return fail(BN_ERR_INVALID, "a K-sharded solve takes one instance per handle");
    if (h && h->p.slip_on) return fail(BN_ERR_INVALID, "K-sharding is not available in sampled-slip mode");
    return solve_impl(h, states, states_where, eps, noise, true);
}

int bn_mppi_shard_partials(bn_mppi_t *h, const float **partials_device, int32_t *workgroups, int32_t *floats_per_workgroup)
{
    if (!h) return fail(BN_ERR_INVALID, "null handle");
    if (!h->shard_pending) return fail(BN_ERR_STATE, "no sharded solve in flight");
    const int cur = (int)((h->solves - 1) % kSlots);
    if (partials_device) *partials_device = h->d_part[cur];
    if (workgroups) *workgroups = h->p.nblk;
    if (floats_per_workgroup) *floats_per_workgroup = 2 + 2 * h->p.T;
    return BN_OK;
}

int bn_mppi_shard_finish_async(bn_mppi_t *h, const float *all_partials_device, int32_t total_workgroups)
{
    if (!h) return fail(BN_ERR_INVALID, "null handle");
    if (!h->shard_pending) return fail(BN_ERR_STATE, "no sharded solve in flight");
    if (!all_partials_device || total_workgroups < h->p.nblk) return fail(BN_ERR_INVALID, "need the partials of every shard");
    BN_BIND(h);
    if (int rc = settle_point(h)) return rc;
    bn::SolveParams p = h->p;
    const int cur = (int)((h->solves - 1) % kSlots);
    p.solve = p.tail_solve = h->solves - 1;
    p.part = const_cast<float *>(all_partials_device);      // merged in shard order: identical on every rank
    p.nblk = total_workgroups;
    p.cost = h->d_cost[cur]; p.state = h->d_state_copy[cur];
    BN_HIP(bn::launch_finish(p, h->stream));                 // weights of the local rollouts, normalised by the global sum
    h->shard_pending = false;
    return BN_OK;
}

}  // extern "C"

// ---- the exchange of a K-sharded solve enqueued by the library: RCCL on the handle's stream -----------------------------------
// Round 4's ShardedMPPI drove the three steps from Python -- launch, torch.distributed.all_gather_into_tensor (its own stream, two
// events to fence it against the planner's), launch: 60 us per solve on one rank against 28 unsharded.  Here the triple is ONE C call
// and ONE queue: rollout kernel, ncclAllGather, tail kernel, stream-ordered, no host wait, no event.  RCCL is opened with dlopen on
// first use: the library has no link-time dependency on it, and a process that never shards a solve never loads it.
namespace {
struct RcclApi {
    void *lib = nullptr;
    decltype(&ncclGetUniqueId) get_unique_id = nullptr;
    decltype(&ncclCommInitRank) comm_init_rank = nullptr;
    decltype(&ncclAllGather) all_gather = nullptr;
    decltype(&ncclCommDestroy) comm_destroy = nullptr;
    decltype(&ncclGetErrorString) error_string = nullptr;
};
const RcclApi *rccl_api()
{
    static const RcclApi api = [] {
        RcclApi a;
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            a.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (a.lib) break;
        }
        if (!a.lib) return a;
        a.get_unique_id = reinterpret_cast<decltype(a.get_unique_id)>(dlsym(a.lib, "ncclGetUniqueId"));
        a.comm_init_rank = reinterpret_cast<decltype(a.comm_init_rank)>(dlsym(a.lib, "ncclCommInitRank"));
        a.all_gather = reinterpret_cast<decltype(a.all_gather)>(dlsym(a.lib, "ncclAllGather"));
        a.comm_destroy = reinterpret_cast<decltype(a.comm_destroy)>(dlsym(a.lib, "ncclCommDestroy"));
        a.error_string = reinterpret_cast<decltype(a.error_string)>(dlsym(a.lib, "ncclGetErrorString"));
        if (!a.get_unique_id || !a.comm_init_rank || !a.all_gather || !a.comm_destroy || !a.error_string) a.lib = nullptr;
        return a;
    }();
    return api.lib ? &api : nullptr;
}
}  // namespace

namespace bn {
namespace host {

void shard_comm_release(bn_mppi *h)
{
    if (h->shard_side) (void)hipStreamSynchronize(h->shard_side);
    if (h->shard_comm) { if (const RcclApi *r = rccl_api()) (void)r->comm_destroy(static_cast<ncclComm_t>(h->shard_comm)); }
    h->shard_comm = nullptr;
    h->shard_prepared = false;
    h->shard_bufs.free_all();
    h->shard_bufs.list.clear();                        // (the next prepare may be for another world size)
    if (h->shard_side_own && h->shard_side) (void)hipStreamDestroy(h->shard_side);
    h->shard_side = nullptr;
}

}  // namespace host
}  // namespace bn

extern "C" {

int bn_dist_unique_id(uint8_t out[BN_DIST_UNIQUE_ID_BYTES])
{
    static_assert(sizeof(ncclUniqueId) == BN_DIST_UNIQUE_ID_BYTES, "ncclUniqueId size");
    if (!out) return fail(BN_ERR_INVALID, "null output");
    const RcclApi *r = rccl_api();
    if (!r) return fail(BN_ERR_HIP, "librccl.so could not be opened: %s", dlerror());
    ncclUniqueId id;
    const ncclResult_t e = r->get_unique_id(&id);
    if (e != ncclSuccess) return fail(BN_ERR_HIP, "ncclGetUniqueId: %s", r->error_string(e));
    std::memcpy(out, &id, sizeof(id));
    return BN_OK;
}

int bn_mppi_shard_comm_prepare(bn_mppi_t *h, int32_t world_size, int32_t rank)
{
    // Everything bn_mppi_shard_comm_init can fail on BEFORE it enters the collective (ncclCommInitRank): opening RCCL, the handle's
    // state, the buffers, events and the side stream.  Local, no communication: the ranks of a job call it, agree on the outcome by
    // whatever means they have (benchnav_amd.sharding: one all-reduce over the torch group), and enter the collective only if every
    // rank is ready -- a rank that cannot must not leave the others waiting in ncclCommInitRank's bootstrap.
    if (!h) return fail(BN_ERR_INVALID, "null argument");
    if (world_size < 1 || rank < 0 || rank >= world_size) return fail(BN_ERR_INVALID, "rank %d outside a world of %d", rank, world_size);
    if (h->p.B != 1 || h->p.slip_on) return fail(BN_ERR_INVALID, "a K-sharded solve takes one instance per handle, without sampled slip");
    if (h->shard_comm) return fail(BN_ERR_STATE, "the handle has a communicator already");
    if ((size_t)world_size * h->p.nblk > 1024) return fail(BN_ERR_INVALID, "the library's exchange merges at most 1024 workgroups (65536 rollouts)");
    if (h->shard_prepared) {
        if (h->shard_world == world_size && h->shard_rank == rank) return BN_OK;
        return fail(BN_ERR_STATE, "the handle was prepared as rank %d of %d", h->shard_rank, h->shard_world);
    }
    const RcclApi *r = rccl_api();
    if (!r) return fail(BN_ERR_HIP, "librccl.so could not be opened: %s", dlerror());
    BN_BIND(h);
    if (int rc = settle_point(h)) return rc;
    // [ kSlots merged rows | 64 group rows | ticket ]
    const size_t merged_floats = kSlots * (2 * (size_t)h->p.T + 2) + 64 * (2 + 2 * (size_t)h->p.T) + 4;
    h->shard_bufs.add(&h->d_gathered, (size_t)world_size * h->p.nblk * (2 + 2 * (size_t)h->p.T) * sizeof(float));
    h->shard_bufs.add(&h->d_shard_merged, merged_floats * sizeof(float));
    h->shard_bufs.add_event(&h->ev_shard_merge, hipEventDisableTiming);
    for (int q = 0; q < kSlots; ++q) h->shard_bufs.add_event(&h->ev_shard_tail[q], hipEventDisableTiming);
    if (int rc = h->shard_bufs.alloc_all(table_fail)) { h->shard_bufs.list.clear(); return rc; }
    h->shard_world = world_size;
    h->shard_rank = rank;
    // the side stream of the tail: the handle's second stream if it has one (overlapped batches), else one of its own
    bool ok = fills_done() == BN_OK;
    if (ok && h->n_streams > 1 && h->xstream[0]) h->shard_side = h->xstream[0];
    else if (ok) { ok = hipStreamCreateWithFlags(&h->shard_side, hipStreamNonBlocking) == hipSuccess; h->shard_side_own = ok; }
    if (!ok) { (void)hipGetLastError(); shard_comm_release(h); return fail(BN_ERR_HIP, "stream / event / buffer creation for the sharded solve failed"); }
    h->shard_prepared = true;
    return BN_OK;
}

int bn_mppi_shard_comm_init(bn_mppi_t *h, const uint8_t unique_id[BN_DIST_UNIQUE_ID_BYTES], int32_t world_size, int32_t rank)
{
    if (!h || !unique_id) return fail(BN_ERR_INVALID, "null argument");
    if (int rc = bn_mppi_shard_comm_prepare(h, world_size, rank)) return rc;      // (a no-op behind the caller's own prepare)
    const RcclApi *r = rccl_api();
    BN_BIND(h);
    ncclUniqueId id;
    std::memcpy(&id, unique_id, sizeof(id));
    ncclComm_t comm = nullptr;
    const ncclResult_t e = r->comm_init_rank(&comm, world_size, id, rank);      // collective: every rank of the solve calls it
    if (e != ncclSuccess) { shard_comm_release(h); return fail(BN_ERR_HIP, "ncclCommInitRank: %s", r->error_string(e)); }
    h->shard_comm = comm;
    return BN_OK;
}

int bn_mppi_shard_solve_async(bn_mppi_t *h, const float *states, bn_mem_kind states_where, const float *eps, bn_noise_kind noise)
{
    if (!h) return fail(BN_ERR_INVALID, "null handle");
    if (!h->shard_comm) return fail(BN_ERR_STATE, "bn_mppi_shard_comm_init must precede bn_mppi_shard_solve_async");
    // The rollouts of THIS solve do not wait for the previous solve's tail on the side stream (flush_tail would join it): they read
    // the mean the merge wrote, on this stream.  And they write their partial rows where the all-gather wants them (in place).
    // Every per-solve buffer rotates over kSlots solves -- the costs and the start state the rollouts below write, the merged row -- and
    // the side-stream tail of the solve kSlots back still reads its slot (weights, cost copy, X*).  That tail is done unless something is
    // badly stuck, so the host LOOKS (hipEventQuery) and only a tail still running puts a cross-queue wait in front of the ROLLOUTS
    // (the check used to sit behind them and covered the merged row only) -- an event wait between queues costs
    // microseconds on the handle's stream even when the event has long fired (first cut of this path: 72 us per solve with an
    // unconditional wait against 47 without the split).
    {
        BN_BIND(h);
        const int next = (int)(h->solves % kSlots);
        if (h->solves >= (uint64_t)kSlots && h->ev_shard_tail[next] && hipEventQuery(h->ev_shard_tail[next]) != hipSuccess) {
            (void)hipGetLastError();
            BN_HIP(hipStreamWaitEvent(h->stream, h->ev_shard_tail[next], 0));
        }
    }
    const bool inflight = h->shard_tail_inflight;
    h->shard_tail_inflight = false;
    h->shard_inplace = true;
    const int rc0 = bn_mppi_shard_rollout_async(h, states, states_where, eps, noise);
    h->shard_inplace = false;
    h->shard_tail_inflight = inflight;
    if (rc0) return rc0;
    BN_BIND(h);
    const int cur = (int)((h->solves - 1) % kSlots);
    const size_t count = (size_t)h->p.nblk * (2 + 2 * (size_t)h->p.T);          // equal shards: every rank contributes the same rows
    const RcclApi *r = rccl_api();
    const ncclResult_t e = r->all_gather(h->d_gathered + (size_t)h->shard_rank * count, h->d_gathered, count, ncclFloat,
                                         static_cast<ncclComm_t>(h->shard_comm), h->stream);
    if (e != ncclSuccess) {
        h->shard_pending = false;                            // the solve is lost, the handle is not: the next call starts a new one
        return fail(BN_ERR_HIP, "ncclAllGather: %s", r->error_string(e));
    }
    // Merge on the handle's stream -- U*, the next mean, the softmin statistics: all the next solve's rollouts wait for -- and the
    // rest of the tail (X* rollout, the shard's weights, the cost copy: ~10 us of one workgroup) on the side stream, beside them.
    // What the two streams share: the outputs (tails stay in order on their one stream; U* is the merge's alone), the per-solve slots
    // of costs / states, and the merged row (written by the merge, read by the tail) -- all rotating over kSlots solves and covered by
    // the look at the tail kSlots back in front of the rollouts, above.
    if (int rc = settle_point(h)) return rc;
    bn::SolveParams p = h->p;
    p.solve = p.tail_solve = h->solves - 1;
    p.part = h->d_gathered;                                  // merged in shard order: identical on every rank
    p.nblk = h->shard_world * h->p.nblk;
    p.cost = h->d_cost[cur]; p.state = h->d_state_copy[cur];
    float *merged = h->d_shard_merged + (size_t)cur * (2 * (size_t)p.T + 2);
    p.ustar_cur = merged; p.stats_cur = merged + 2 * (size_t)p.T;
    float *group_rows = h->d_shard_merged + kSlots * (2 * (size_t)p.T + 2);
    BN_HIP(bn::launch_shard_merge(p, group_rows, reinterpret_cast<int *>(group_rows + 64 * (2 + 2 * (size_t)p.T)), h->stream));
    BN_HIP(hipEventRecord(h->ev_shard_merge, h->stream));
    BN_HIP(hipStreamWaitEvent(h->shard_side, h->ev_shard_merge, 0));
    p.tail_merged = 1;
    p.ustar_written = 1;                                     // (the merge kernel above wrote U*: see SolveParams::ustar_written)
    p.ustar_prev = merged; p.stats_prev = merged + 2 * (size_t)p.T;
    BN_HIP(bn::launch_finish(p, h->shard_side));            // weights of the local rollouts, normalised by the global sum; X*
    BN_HIP(hipEventRecord(h->ev_shard_tail[cur], h->shard_side));
    h->shard_tail_slot = cur;
    h->shard_tail_inflight = true;
    h->shard_pending = false;
    return BN_OK;
}

}  // extern "C"
