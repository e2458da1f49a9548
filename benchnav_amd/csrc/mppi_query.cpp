// mppi_query.cpp -- what the C ABI hands back: the getters (copies, re-rolled rows, top samples, device buffers), the event
// profiling, the byte counts bench.py reports, and the lab hooks (device math / RNG evaluation, BN_TIMING switches).
#include "mppi_handle.h"

#include <algorithm>
#include <numeric>
#include <vector>

using namespace bn::host;

extern "C" {

int bn_mppi_get_mean(bn_mppi_t *h, int32_t instance, float *mean_host)
{
    if (int rc = check_instance(h, instance, false)) return rc;
    if (!mean_host) return fail(BN_ERR_INVALID, "null output");
    BN_BIND(h);
    if (int rc = settle_point(h)) return rc;
    if (int rc = flush_tail(h)) return rc;
    BN_HIP(hipStreamSynchronize(h->stream));
    const size_t n = (size_t)h->p.T * 2;
    BN_HIP(hipMemcpy(mean_host, h->d_mean + instance * n, n * 4, hipMemcpyDeviceToHost));
    return BN_OK;
}

// Rows of the latest solve's trajectory batch, regenerated (launch_reroll).  The tail of that solve must have run
// (mean_used, state copy); the caller's eps block of that solve must still be alive when the noise was injected.
static int reroll_rows(bn_mppi_t *h, int32_t instance, const int *idx_device, int32_t n, float *out_device)
{
    if (h->p.slip_on) return fail(BN_ERR_INVALID, "re-rolling is not available in sampled-slip mode");
    if (h->solves == 0) return fail(BN_ERR_STATE, "no solve has run");
    if (h->shard_pending) return fail(BN_ERR_STATE, "a sharded solve waits for bn_mppi_shard_finish_async");
    // The rows are rolled out again on the map as it is NOW: after a bn_mppi_set_map they would not be the latest solve's rollouts
    // (the reference's get_top_samples returns the batch forward() stored, mppi.py:221-240) -- refuse instead of answering for another map.
    if (h->map_epoch != h->map_epoch_at_solve)
        return fail(BN_ERR_STATE, "the map changed since the latest solve: its rollouts cannot be regenerated (read them before bn_mppi_set_map, or solve again)");
    if (int rc = flush_tail(h)) return rc;
    bn::SolveParams p = h->p;
    const int cur = (int)((h->solves - 1) % kSlots);
    p.solve = h->solves - 1;
    p.state = h->d_state_copy[cur];
    p.eps = h->last_eps;
    if (int rc = guard_foreign_overlap(h)) return rc;
    BN_HIP(bn::launch_reroll(p, h->last_mode, instance, idx_device, n, out_device, h->stream));
    return BN_OK;
}

int bn_mppi_reroll_async(bn_mppi_t *h, int32_t instance, const int32_t *idx_device, int32_t n, float *out_device)
{
    if (int rc = check_instance(h, instance, false)) return rc;
    if (n < 0 || (!idx_device && n > h->p.K)) return fail(BN_ERR_INVALID, "n=%d out of range", n);
    if (n == 0) return BN_OK;
    if (!out_device) return fail(BN_ERR_INVALID, "null output");
    BN_BIND(h);
    if (int rc = settle_point(h)) return rc;
    return reroll_rows(h, instance, idx_device, n, out_device);
}

static int copy_out(bn_mppi_t *h, int32_t instance, const float *dev, size_t per_instance, float *out_host)
{
    if (int rc = check_instance(h, instance, false)) return rc;
    if (!out_host) return fail(BN_ERR_INVALID, "null output");
    BN_BIND(h);
    if (int rc = settle_point(h)) return rc;
    if (int rc = flush_tail(h)) return rc;
    BN_HIP(hipStreamSynchronize(h->stream));
    BN_HIP(hipMemcpy(out_host, dev + (size_t)instance * per_instance, per_instance * 4, hipMemcpyDeviceToHost));
    return BN_OK;
}

int bn_mppi_get_weights(bn_mppi_t *h, int32_t instance, float *out_host)
{
    return h ? copy_out(h, instance, h->d_w, h->p.K, out_host) : fail(BN_ERR_INVALID, "null handle");
}

int bn_mppi_get_costs(bn_mppi_t *h, int32_t instance, float *out_host)
{
    return h ? copy_out(h, instance, h->d_cost_out, h->p.K, out_host) : fail(BN_ERR_INVALID, "null handle");
}

int bn_mppi_get_states(bn_mppi_t *h, int32_t instance, float *out_host)
{
    if (int rc = check_instance(h, instance, false)) return rc;
    if (!out_host) return fail(BN_ERR_INVALID, "null output");
    BN_BIND(h);
    if (int rc = settle_point(h)) return rc;
    const size_t K = h->p.K, Kp = h->p.Kp, T1 = h->p.T + 1, n = K * T1 * 3;
    if (int rc = ensure_scratch(h, n * 4)) return rc;
    if (h->p.lean) {                                   // not materialised: regenerate all K rows
        if (int rc = reroll_rows(h, instance, nullptr, (int32_t)K, h->d_scratch)) return rc;
    } else
    BN_HIP(bn::launch_states_to_reference((h->x_idx && h->d_Xalt[0] ? h->d_Xalt[0] : h->d_X) + (size_t)instance * Kp * T1 * 3, h->d_scratch, (int)K, (int)Kp, (int)T1,
                                          h->stream));
    BN_HIP(hipMemcpyAsync(out_host, h->d_scratch, n * 4, hipMemcpyDeviceToHost, h->stream));
    BN_HIP(hipStreamSynchronize(h->stream));
    return BN_OK;
}

int bn_mppi_get_controls(bn_mppi_t *h, int32_t instance, float *out_host)
{
    if (int rc = check_instance(h, instance, false)) return rc;
    if (!out_host) return fail(BN_ERR_INVALID, "null output");
    if (!h->d_U || !h->p.store_u) return fail(BN_ERR_STATE, "controls are only stored with BN_FLAG_STORE_CONTROLS");
    BN_BIND(h);
    if (int rc = settle_point(h)) return rc;
    const size_t K = h->p.K, Kp = h->p.Kp, T = h->p.T, n = K * T * 2;
    if (int rc = ensure_scratch(h, n * 4)) return rc;
    BN_HIP(bn::launch_controls_to_reference((h->x_idx && h->d_Ualt[0] ? h->d_Ualt[0] : h->d_U) + (size_t)instance * Kp * T * 2, h->d_scratch, (int)K, (int)Kp, (int)T,
                                            h->stream));
    BN_HIP(hipMemcpyAsync(out_host, h->d_scratch, n * 4, hipMemcpyDeviceToHost, h->stream));
    BN_HIP(hipStreamSynchronize(h->stream));
    return BN_OK;
}

int bn_mppi_get_philox_noise(bn_mppi_t *h, int32_t instance, uint64_t solve_index, float *out_host)
{
    if (int rc = check_instance(h, instance, false)) return rc;
    if (!out_host) return fail(BN_ERR_INVALID, "null output");
    BN_BIND(h);
    if (int rc = settle_point(h)) return rc;
    const size_t n = (size_t)h->p.K * h->p.T * 2;
    if (int rc = ensure_scratch(h, n * 4)) return rc;
    BN_HIP(bn::launch_philox_noise(h->d_scratch, h->p.seed, solve_index, instance, h->p.K, h->p.T, h->p.k0, h->stream));
    BN_HIP(hipMemcpyAsync(out_host, h->d_scratch, n * 4, hipMemcpyDeviceToHost, h->stream));
    BN_HIP(hipStreamSynchronize(h->stream));
    return BN_OK;
}

int bn_mppi_get_slip_noise(bn_mppi_t *h, int32_t instance, uint64_t solve_index, float *zt_host, float *zc_host, float *zo_host)
{
    if (int rc = check_instance(h, instance, false)) return rc;
    if (!zt_host || !zc_host || !zo_host) return fail(BN_ERR_INVALID, "null output");
    if (!h->p.slip_on) return fail(BN_ERR_STATE, "handle was created without BN_FLAG_SAMPLED_SLIP");
    BN_BIND(h);
    const size_t K = h->p.K, T = h->p.T, nt = K * T, nc = K * (T + 1);
    if (int rc = ensure_scratch(h, (nt + nc + T) * 4)) return rc;
    float *zt = h->d_scratch, *zc = zt + nt, *zo = zc + nc;
    BN_HIP(bn::launch_philox_slip(zt, zc, zo, h->p.seed, solve_index, instance, (int)K, (int)T, h->p.k0, h->stream));
    BN_HIP(hipMemcpyAsync(zt_host, zt, nt * 4, hipMemcpyDeviceToHost, h->stream));
    BN_HIP(hipMemcpyAsync(zc_host, zc, nc * 4, hipMemcpyDeviceToHost, h->stream));
    BN_HIP(hipMemcpyAsync(zo_host, zo, T * 4, hipMemcpyDeviceToHost, h->stream));
    BN_HIP(hipStreamSynchronize(h->stream));
    return BN_OK;
}

int bn_mppi_get_top_samples(bn_mppi_t *h, int32_t instance, int32_t n, float *states_host, float *weights_host)
{
    if (int rc = check_instance(h, instance, false)) return rc;
    if (n < 0 || n > h->p.K) return fail(BN_ERR_INVALID, "n=%d must satisfy 0 <= n <= K=%d", n, h->p.K);  // mppi.py:229
    if (n == 0) return BN_OK;
    if (!states_host || !weights_host) return fail(BN_ERR_INVALID, "null output");
    BN_BIND(h);
    if (int rc = settle_point(h)) return rc;
    const size_t K = h->p.K, T1 = h->p.T + 1;
    std::vector<float> w(K);
    if (int rc = flush_tail(h)) return rc;
    BN_HIP(hipStreamSynchronize(h->stream));
    BN_HIP(hipMemcpy(w.data(), h->d_w + (size_t)instance * K, K * 4, hipMemcpyDeviceToHost));
    std::vector<int> idx(K);
    std::iota(idx.begin(), idx.end(), 0);
    // topk + descending sort (mppi.py:232-238); ties resolved by the lower rollout index
    std::partial_sort(idx.begin(), idx.begin() + n, idx.end(),
                      [&](int a, int b) { return w[a] > w[b] || (w[a] == w[b] && a < b); });
    if ((size_t)n > h->idx_count) {
        h->idx_count = 0;
        if (int rc = h->bufs.resize(&h->d_idx, (size_t)n * sizeof(int), table_fail)) return rc;
        if (int rc = fills_done()) return rc;
        h->idx_count = n;
    }
    if (int rc = ensure_scratch(h, (size_t)n * T1 * 3 * 4)) return rc;
    BN_HIP(hipMemcpyAsync(h->d_idx, idx.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, h->stream));
    if (h->p.lean) {                                   // the n winners are re-rolled, bit-identical to a stored batch
        if (int rc = reroll_rows(h, instance, h->d_idx, n, h->d_scratch)) return rc;
    } else
    BN_HIP(bn::launch_gather_states((h->x_idx && h->d_Xalt[0] ? h->d_Xalt[0] : h->d_X) + (size_t)instance * h->p.Kp * T1 * 3, h->d_idx, h->d_scratch, n, h->p.Kp,
                                    (int)T1, h->stream));
    BN_HIP(hipMemcpyAsync(states_host, h->d_scratch, (size_t)n * T1 * 3 * 4, hipMemcpyDeviceToHost, h->stream));
    BN_HIP(hipStreamSynchronize(h->stream));
    for (int i = 0; i < n; ++i) weights_host[i] = w[idx[i]];
    return BN_OK;
}

int bn_mppi_device_buffer(bn_mppi_t *h, bn_buffer_id id, void **device_ptr, size_t *bytes)
{
    if (!h || !device_ptr) return fail(BN_ERR_INVALID, "null argument");
    if (h->shard_tail_inflight) {                     // a library-enqueued sharded solve: order the handle's stream behind its tail first
        BN_BIND(h);
        if (int rc = flush_tail(h)) return rc;
    }
    if ((int)id < 0 || id >= BN_BUF_COUNT_) return fail(BN_ERR_INVALID, "unknown buffer id %d", (int)id);
    // The handle's table answers by id; U* and X* are the two halves of the one BN_BUF_USTAR_XSTAR block.  The size is the plan's,
    // which the table was filled from -- also for a buffer this configuration does not have.
    void *ptr = nullptr;
    size_t block = 0;
    h->bufs.find(id == BN_BUF_USTAR || id == BN_BUF_XSTAR ? BN_BUF_USTAR_XSTAR : id, &ptr, &block);
    if (ptr && id == BN_BUF_XSTAR) ptr = h->d_xstar;
    *device_ptr = ptr;
    if (bytes) *bytes = h->plan_bytes[id];
    if (!ptr) return fail(BN_ERR_STATE, "buffer %d is not allocated in this configuration", (int)id);
    return BN_OK;
}

int32_t bn_mppi_host_paced(const bn_mppi_t *h) { return h ? (h->hp_enabled ? (h->req_bar ? 2 : 1) : 0) : -1; }
int32_t bn_mppi_states_buffer_index(const bn_mppi_t *h) { return h ? h->x_idx : -1; }

int32_t bn_mppi_arithmetic(const bn_mppi_t *h) { return h ? h->p.ref_order : -1; }
int32_t bn_mppi_fast_quotient(const bn_mppi_t *h) { return h ? (h->p.pow2 ? 2 : h->p.fast_div) : -1; }
int32_t bn_mppi_launches_per_solve(const bn_mppi_t *h) { return h ? ((h->pipelined || h->ticket_mode) ? 1 : 2) : -1; }
int32_t bn_mppi_launches_per_forward(const bn_mppi_t *h)
{
    return h ? ((h->lat_kernel && h->pipelined && !h->self_off && !(h->cfg.flags & BN_FLAG_NO_PIPELINE)) ? 1 : 2) : -1;
}

int32_t bn_mppi_row_pitch(const bn_mppi_t *h) { return h ? h->p.Kp : 0; }

int bn_mppi_kernel_ms(bn_mppi_t *h, float *rollout_ms, float *finish_ms, int32_t *n_solves)
{
    if (!h) return fail(BN_ERR_INVALID, "null handle");
    if (!(h->cfg.flags & BN_FLAG_PROFILE)) return fail(BN_ERR_STATE, "handle was created without BN_FLAG_PROFILE");
    BN_BIND(h);
    if (int rc = settle_point(h)) return rc;
    if (h->pipelined || h->ticket_mode) {
        // close the open group with one more event *before* the flush, then average complete groups only
        const int open = h->prof_in_group;
        if (h->ev_used + 1 > h->ev.size()) {
            hipEvent_t e;
            BN_HIP(hipEventCreate(&e));
            h->ev.push_back(e);
        }
        BN_HIP(hipEventRecord(h->ev[h->ev_used++], h->stream));
        if (int rc = flush_tail(h)) return rc;
        BN_HIP(hipStreamSynchronize(h->stream));
        const size_t marks = h->ev_used;                  // marks-1 intervals; the last one holds `open` launches (or a full group)
        double tot = 0.0;
        size_t launches = 0;
        for (size_t i = 0; i + 1 < marks; ++i) {
            const bool last = (i + 2 == marks);
            const int in_this = (last && open != 0) ? open : kProfGroup;
            if (last && open != 0) break;                 // skip the ragged last group
            float a = 0.0f;
            BN_HIP(hipEventElapsedTime(&a, h->ev[i], h->ev[i + 1]));
            tot += a;
            launches += in_this;
        }
        if (rollout_ms) *rollout_ms = launches ? (float)(tot / launches) : 0.0f;
        if (finish_ms) *finish_ms = 0.0f;
        if (n_solves) *n_solves = (int32_t)launches;
        h->ev_used = 0;
        h->prof_in_group = 0;
        return BN_OK;
    }
    if (int rc = flush_tail(h)) return rc;
    BN_HIP(hipStreamSynchronize(h->stream));
    double r = 0.0, f = 0.0;
    const size_t n = h->ev_used / 3;
    for (size_t i = 0; i < n; ++i) {
        float a = 0.0f, b = 0.0f;
        BN_HIP(hipEventElapsedTime(&a, h->ev[3 * i], h->ev[3 * i + 1]));
        BN_HIP(hipEventElapsedTime(&b, h->ev[3 * i + 1], h->ev[3 * i + 2]));
        r += a; f += b;
    }
    if (rollout_ms) *rollout_ms = n ? (float)(r / n) : 0.0f;
    if (finish_ms) *finish_ms = n ? (float)(f / n) : 0.0f;
    if (n_solves) *n_solves = (int32_t)n;
    h->ev_used = 0;
    return BN_OK;
}

int64_t bn_mppi_algorithmic_bytes(const bn_mppi_t *h, bn_noise_kind noise)
{
    if (!h) return 0;
    const int64_t K = h->p.K, T = h->p.T, G = h->p.G;
    int64_t bytes = 4 * G * G            // risk map read once
                    + (8 * T + 12)       // mean, state
                    + (h->p.lean ? 0 : 12 * K * (T + 1))   // _state_seq_batch write (not in lean mode)
                    + 4 * K              // weights write
                    + 8 * T + 12 * (T + 1);   // U*, X* write
    if (noise != BN_NOISE_PHILOX) bytes += 8 * K * T;   // injected noise read
    if (h->p.store_u) bytes += 8 * K * T;               // _perturbed_action_seqs write
    return bytes;
}

/* The same with the map term replaced by what a solve can reach: the LDS window of (WN x WN) cells around the start state, staged
 * once per instance in the best case (every rollout workgroup stages its own copy; the copies hit in L2).  With BN_FLAG_LEAN the
 * map read is most of SURVEY 8d's lean formula, and a kernel that reads the window only would be credited for bytes it never
 * moves: bench.py reports both fractions. */
int64_t bn_mppi_algorithmic_bytes_window(const bn_mppi_t *h, bn_noise_kind noise)
{
    if (!h) return 0;
    const int64_t G = h->p.G, W = h->p.WN > 0 ? h->p.WN : G;
    return bn_mppi_algorithmic_bytes(h, noise) - 4 * G * G + 4 * W * W;
}

#ifdef BN_TIMING
int bn_mppi_debug_blocks_per_cu(bn_mppi_t *h) { return bn::rollout_blocks_per_cu(h->p); }
/* tools/ablate.py only: device buffer of >= 16 uint64 for the in-kernel cycle stamps */
void bn_mppi_debug_set_stamps(bn_mppi_t *h, void *device_ptr) { h->p.stamps = (unsigned long long *)device_ptr; }
void bn_mppi_debug_trace_by_parity(bn_mppi_t *h, int on) { h->p.trace_by_parity = on; }
#endif

int bn_device_math_eval(int32_t fn, const float *in_device, float *out_device, int64_t n, void *stream)
{
    if (fn < 0 || fn > 6 || !in_device || !out_device || n < 0) return fail(BN_ERR_INVALID, "bad argument");
    if (n == 0) return BN_OK;
    BN_HIP(bn::launch_math_eval(fn, in_device, out_device, (size_t)n, (hipStream_t)stream));
    return BN_OK;
}

int bn_device_rng_eval(int32_t fn, const uint32_t *in_device, uint32_t *out_device, int64_t n, void *stream)
{
    if (fn < 0 || fn > 2 || !in_device || !out_device || n < 0) return fail(BN_ERR_INVALID, "bad argument");
    if (n == 0) return BN_OK;
    BN_HIP(bn::launch_rng_eval(fn, in_device, out_device, (size_t)n, (hipStream_t)stream));
    return BN_OK;
}

}  // extern "C"
