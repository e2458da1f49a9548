// mppi_plan.cpp -- plan_mppi: what bn_mppi_create decides (mppi_plan.h), in the order it has always decided it, and the test
// hook that shows the plan without a device (bn_mppi_debug_plan).  No HIP call in this file.
#include "mppi_plan.h"

#include <algorithm>
#include <cmath>

namespace bn {
namespace host {

// Role kernel or one-wave throughput kernel for a many-instance launch?  Both give bit-identical results; which one is faster
// depends on the horizon (the role kernel's skeleton -- prologue, barriers, epilogue -- is a fixed cost per workgroup, the one-wave
// kernel pays per step), on the workgroups per instance (both re-merge nblk rows per workgroup) and on how full the chip gets.
// A two-term estimate of either kernel's time per launch, fitted to tools/auto_sweep.py (K 128..2048, T 10..100, 16..300
// instances, overlapped launches): it picks the faster kernel or one within 10 % of it in 51 of 52 cells (worst: 28 %), where a
// fixed workgroup-count threshold lost 14-60 % in seven.  K=1024, T=50: crossover between 64 and 128 instances as measured.
static bool wave_kernel_is_faster(const bn::SolveParams &p, size_t resident_role_wgs, int n_cus)
{
    const double W = (double)p.B * (p.nblk + 1), R = (double)std::max<size_t>(resident_role_wgs, 1), rows = std::max(0, p.nblk - 16);
    const double role = (4.5 + 0.19 * p.T + 0.3 * rows) * (1.0 + 0.175 * std::min(W, R) / std::max(n_cus, 1)) * std::max(1.0, W / R);
    // (round 5: x 0.93 -- the one-wave kernel lost a quarter of its instructions; re-checked against tools/auto_sweep.py, which had
    // flagged K=1024 T=50 at 80 instances and K=512 T=20 at 128 where the role kernel spills into a second residency round)
    // (not for short horizons or more than 16 workgroups per instance, where the sweep has the role kernel ahead at the old crossover)
    const double gain = (rows == 0 && p.T >= 20) ? 0.93 : 1.0;
    const double wave = gain * (3.3 + 0.44 * p.T + 0.37 * rows) * (1.0 + 1.5 * W / (24.0 * std::max(n_cus, 1)));
    return wave < role;
}

static bool is_pow2_float(float v)
{
    int ex;
    return v > 0.0f && std::isfinite(v) && std::frexp(v, &ex) == 0.5f;
}

int plan_mppi(const bn_mppi_config &config, int n_cus, MppiPlan *out)
{
    const bn_mppi_config *cfg = &config;
    if (cfg->struct_size != sizeof(bn_mppi_config))
        return fail(BN_ERR_INVALID, "bn_mppi_config.struct_size %u != %zu (ABI mismatch)", cfg->struct_size,
                    sizeof(bn_mppi_config));
    if (cfg->horizon < 1 || cfg->num_samples < 1 || cfg->num_instances < 1 || cfg->grid_size < 1)
        return fail(BN_ERR_INVALID, "horizon, num_samples, num_instances and grid_size must be >= 1");
    if (cfg->num_instances > 32768) return fail(BN_ERR_INVALID, "num_instances must be <= 32768");
    if ((cfg->flags & BN_FLAG_LEAN) && (cfg->flags & BN_FLAG_SAMPLED_SLIP))
        return fail(BN_ERR_INVALID, "BN_FLAG_LEAN is not available in sampled-slip mode");
    if (!(cfg->resolution > 0.0f) || !(cfg->lambda_ > 0.0f) || !(cfg->dt > 0.0f))
        return fail(BN_ERR_INVALID, "resolution, lambda_ and dt must be positive");
    for (int d = 0; d < 2; ++d)
        if (!(cfg->u_min[d] <= cfg->u_max[d]) || !(cfg->sigma[d] >= 0.0f))
            return fail(BN_ERR_INVALID, "need u_min <= u_max and sigma >= 0");
    // The default arithmetic carries the heading vector by a small-angle rotation per step (rotate_spec, bn_device_math.h): its
    // degree-6 polynomials are good to 1e-7 up to 0.5 rad per step (the reference's dt = 0.1, |omega| <= 1 give 0.1), and the
    // branch-free near form of the heading wrap needs less than pi.  The reference itself has no such bound (transit takes any
    // delta_t, robot_model.py:60): beyond it the handle takes the reference-order arithmetic -- sincos_spec of every step's heading,
    // general wrap -- exactly as if BN_FLAG_REFERENCE_ORDER had been given (bn_mppi_arithmetic() tells).
    const bool big_step = !((double)cfg->dt * std::max(std::fabs((double)cfg->u_min[1]), std::fabs((double)cfg->u_max[1])) <= 0.5);
    if (big_step && !std::isfinite((double)cfg->dt * ((double)cfg->u_max[1] - (double)cfg->u_min[1])))
        return fail(BN_ERR_INVALID, "dt and the angular-velocity bounds must be finite");
    // The kernels share one gather between stage cost t and transit t+1; that needs the upper clamp
    // to land in the last cell, as it does for every reference GridMap (grid_map.py:42-50).
    const float span_x = (cfg->x_limits[1] - cfg->x_limits[0]) / cfg->resolution;
    const float span_y = (cfg->y_limits[1] - cfg->y_limits[0]) / cfg->resolution;
    if (!(span_x >= (float)(cfg->grid_size - 1)) || !(span_y >= (float)(cfg->grid_size - 1)))
        return fail(BN_ERR_INVALID, "x/y_limits must span at least grid_size-1 cells of `resolution`");

    MppiPlan plan{};
    MppiPlan *h = &plan;
    h->struct_size = sizeof(bn_mppi_plan_info);
    h->n_cus = std::max(n_cus, 1);
    h->n_streams = 1;
    bn::SolveParams &p = h->p;
    p.K = cfg->num_samples; p.T = cfg->horizon; p.G = cfg->grid_size; p.B = cfg->num_instances;
    p.nblk = (p.K + bn::kRolloutsPerBlock - 1) / bn::kRolloutsPerBlock;
    p.Kp = p.nblk * bn::kRolloutsPerBlock;
    p.res = cfg->resolution; p.inv_res = 1.0f / cfg->resolution;
    p.pow2 = is_pow2_float(cfg->resolution) ? 1 : 0;
    p.x0 = cfg->x_limits[0]; p.y0 = cfg->y_limits[0];
    p.x_hi = cfg->x_limits[1]; p.y_hi = cfg->y_limits[1];
    p.dt = cfg->dt; p.thr = cfg->stuck_threshold; p.lambda_ = cfg->lambda_;
    {
        int e = 0;
        const float m = std::frexp(cfg->lambda_, &e);                  // lambda_ = m * 2^e, m in [0.5, 1)
        p.inv_lambda = (m == 0.5f && e > -120 && e < 120) ? std::ldexp(1.0f, 1 - e) : 0.0f;
    }
    p.sigma0 = cfg->sigma[0]; p.sigma1 = cfg->sigma[1];
    p.iv0 = cfg->inv_var[0]; p.iv1 = cfg->inv_var[1];
    p.umin0 = cfg->u_min[0]; p.umax0 = cfg->u_max[0];
    p.umin1 = cfg->u_min[1]; p.umax1 = cfg->u_max[1];
    p.seed = cfg->seed;
    p.store_u = (cfg->flags & BN_FLAG_STORE_CONTROLS) ? 1 : 0;
    p.lean = (cfg->flags & BN_FLAG_LEAN) ? 1 : 0;
    // One-wave kernel, library noise: how much of the horizon the epilogue draws again instead of reading the controls back (see
    // rollout_wave.inc).  Everything with the trajectory dump (its stores already load the memory system), nothing in lean mode.
    p.regen_steps = p.T;
    p.park_steps = bn::kWaveParkSteps;
    if (const char *e = exp_env("BN_REGEN_STEPS")) p.regen_steps = std::max(0, atoi(e));      // experiments: tools/wave_ab.py
    if (const char *e = exp_env("BN_PARK_STEPS")) p.park_steps = std::min(std::max(0, atoi(e)), bn::kWaveParkSteps);
    p.lds_park = 0;                                    // decided below, when the window is known
    p.ref_order = ((cfg->flags & BN_FLAG_REFERENCE_ORDER) || big_step) ? 1 : 0;
    p.wrap_near = ((double)cfg->dt * std::max(std::fabs((double)cfg->u_min[1]), std::fabs((double)cfg->u_max[1])) < 3.0) ? 1 : 0;
    // Workgroup i of a launch runs on XCD i % 8 (observed, used for speed only).  xs = 3 interleaves 8 instances along grid x
    // so that the workgroups of one instance share an XCD's L2 (rollout_grid); measured SLOWER (64 instances: 29.2 vs 28.1 us,
    // 60: 28.5 vs 24.9): the dispatcher then fills the CUs unevenly (3 to 5 workgroups per CU instead of 4, tools/block_trace.py)
    // and a few workgroups wait for a second round.  Default: instance per grid row, workgroups of an instance spread over the XCDs.
    p.xs = 0;
    if (const char *e = exp_env("BN_XCD_PACK")) p.xs = (e[0] == '1') ? 3 : 0;      // experiments (tools/r2_measure.py)

    h->n_maps = (cfg->flags & BN_FLAG_SHARED_MAP) ? 1 : p.B;
    p.map_stride = (h->n_maps == 1) ? 0 : p.G * p.G;

    // Reachable window: |dx| per step <= trav*|v|*dt <= vmax*dt (robot_model.py:82,86-87).
    const double vmax = std::max(std::fabs((double)cfg->u_min[0]), std::fabs((double)cfg->u_max[0]));
    const double reach_cells = std::ceil((double)p.T * vmax * (double)cfg->dt / (double)cfg->resolution) + 1.0;
    p.reach = (int)std::min(reach_cells, (double)p.G);
    // reach either side of the start cell (reach has a cell to spare), up to the whole map plus the guard row / column at index G
    // (window_origin_wide).  An odd pitch on purpose: with 2 reach + 2 vertically adjacent cells collided in the LDS banks more
    // often (K=16384 T=100: 27.4 -> 28.5 us per solve).
    p.WN = std::min(p.G + 1, 2 * p.reach + 1);
    const size_t lds_budget = 160 * 1024;
    // The clamp-free window gather (trav_window) relies on the raw cell of an in-limits position being <= G, the guard row / column:
    // true for every reference GridMap (limits span exactly G cells, grid_map.py:42-50).  Limits that span MORE cells than the grid
    // has put raw cells beyond the guard for positions clamped to the upper limit; such a geometry takes the clamped gather from
    // global memory (the reference's index clamp, grid_map.py:209), like BN_FLAG_NO_LDS_WINDOW.
    const bool wide_limits = span_x > (float)cfg->grid_size * (1.0f + 1e-6f) || span_y > (float)cfg->grid_size * (1.0f + 1e-6f);
    if ((cfg->flags & BN_FLAG_NO_LDS_WINDOW) || wide_limits) p.WN = 0;
    // Slow path: a horizon whose control tile does not fit the role kernels' LDS (MPPI.__init__ takes any horizon, mppi.py:25), or
    // the reference-order arithmetic in sampled-slip mode (its fused kernel has no such variant).  The one-wave kernel keeps its
    // controls in HBM and has no tile: rollouts + stand-alone tail, two launches per solve, one stream.  (The reference order by
    // itself runs on every kernel: rollout_role_ref_*.hip, rollout_wave_ref.hip.)
    h->slow_path = p.ref_order != 0 && (cfg->flags & BN_FLAG_SAMPLED_SLIP) != 0;
    if (!h->slow_path) {
        if (bn::rollout_lds_bytes(p) > lds_budget) p.WN = 0;
        if (bn::rollout_lds_bytes(p) > lds_budget) { h->slow_path = true; p.WN = wide_limits || (cfg->flags & BN_FLAG_NO_LDS_WINDOW) ? 0 : std::min(p.G + 1, 2 * p.reach + 1); }
    }
    // Sampled slip: the tail's optimal rollout stages a (mean, std) window on top of the plain one -- three windows' worth of LDS.  A
    // reach that fits the rollout kernels (which fall back to the global gather by themselves, sampled_fused) can still be too much
    // for the tail; then everything gathers from global memory.  (Round 4: tools/fuzz_sweep.py, seed 2327 -- T = 63, 0.1 m cells,
    // 1 m/s: a 129 x 129 window, 200 KB in the tail, and the launch failed with "invalid argument".)
    if ((cfg->flags & BN_FLAG_SAMPLED_SLIP) && !h->slow_path && bn::finish_lds_bytes_for(p, true) > lds_budget) p.WN = 0;
    if (h->slow_path) {
        const bool sampled = (cfg->flags & BN_FLAG_SAMPLED_SLIP) != 0;
        if (bn::wave_lds_bytes(p) > lds_budget || (sampled && bn::finish_lds_bytes_for(p, true) > lds_budget)) p.WN = 0;
        const size_t need = sampled ? sizeof(float) * (4 * (size_t)p.T + 2 * (size_t)p.T * bn::kUPad + 64) : bn::wave_lds_bytes(p);
        if (need > lds_budget || bn::finish_lds_bytes_for(p, sampled) > lds_budget)
            return fail(BN_ERR_INVALID, "horizon %d needs %zu B of LDS even on the slow path (> 160 KiB)", p.T, std::max(need, bn::finish_lds_bytes_for(p, sampled)));
    }

    {
        const size_t by_lds = lds_budget / std::max<size_t>(bn::rollout_lds_bytes(p), 1);
        const size_t by_waves = 32 / (bn::kRolloutThreads / 64);
        h->resident_wgs = std::max<size_t>(1, std::min(by_lds, by_waves)) * (size_t)h->n_cus;
    }
    h->has_X = !p.lean;                                // lean mode never materialises _state_seq_batch
    // the throughput kernel keeps its controls in this buffer instead of an LDS tile, requested or not
    h->want_wave = !h->slow_path && !(cfg->flags & (BN_FLAG_NO_PIPELINE | BN_FLAG_ROLE_KERNEL | BN_FLAG_SAMPLED_SLIP)) && p.nblk <= 32 &&
                   ((cfg->flags & BN_FLAG_WAVE_KERNEL) ||
                    (((size_t)p.B + 1) * (p.nblk + 1) > (size_t)h->n_cus && wave_kernel_is_faster(p, h->resident_wgs, h->n_cus)));
    h->has_U = p.store_u || h->want_wave || h->slow_path;
    // one-wave kernel: a second control tile in LDS for the chunk behind the register block, if 16 workgroups per CU still fit
    if (h->want_wave && p.park_steps > 0 && p.regen_steps > 0 && p.WN > 0 && !exp_env("BN_NO_LDS_PARK")) {
        p.lds_park = 1;
        if (bn::wave_lds_bytes(p) > (size_t)160 * 1024 / 16) p.lds_park = 0;
    }
    // every rollout workgroup re-merges the previous solve's nblk partials: only worth it while they are few
    p.slip_on = (cfg->flags & BN_FLAG_SAMPLED_SLIP) ? 1 : 0;
    // (the fused sampled-slip kernel has its own, larger LDS layout: what an overlapped batch may count on being resident -- the
    // residency rules of bn_mppi_solve_n_async -- is that kernel's figure, not the role kernel's)
    if (p.slip_on && bn::sampled_fused(p)) h->resident_wgs = bn::sampled_resident_per_cu(p) * (size_t)h->n_cus;
    h->pipelined = !h->slow_path && !(cfg->flags & BN_FLAG_NO_PIPELINE) && p.nblk <= kPipelinedMaxBlocks && !p.slip_on;
    // throughput kernel: launches with more workgroups than the role kernel keeps resident in one round (4 per CU)
    h->wave_kernel = h->pipelined && h->want_wave;
    // latency variant: every workgroup (rollouts + aux) alone on a CU -- with room left for one instance of an overlapped successor
    // (15 instances of K=1024 fill 255 of 256 CUs: 15.3 us per launch against the role kernel's 13.9; 14 instances 13.1 against
    // 13.9) --, its LDS layout must fit, not forced elsewhere
    h->lat_kernel = h->pipelined && !h->wave_kernel && !(cfg->flags & BN_FLAG_ROLE_KERNEL) && bn::lat_lds_bytes(p) > 0 &&
                    ((cfg->flags & BN_FLAG_LAT_KERNEL) || ((size_t)p.B + 1) * (p.nblk + 1) <= (size_t)h->n_cus);
    if (const char *e = exp_env("BN_LAT_KERNEL")) h->lat_kernel = h->lat_kernel && e[0] != '0';      // experiments
    h->has_granules = h->lat_kernel && p.nblk <= 16 && 2 * p.T <= bn::kRolloutThreads && !exp_env("BN_NO_GRANULES");
    // the role kernel (launches that do not leave every workgroup a CU of its own) overlaps its launches as well: a workgroup of
    // the next solve takes the slot a finished one frees and waits there for ITS instance's previous solve only
    h->role_overlap = h->pipelined && !h->lat_kernel && !(cfg->flags & BN_FLAG_NO_OVERLAP);
    if (const char *e = exp_env("BN_ROLE_OVERLAP")) h->role_overlap = h->role_overlap && e[0] != '0';   // experiments
    // the deterministic kernel's ticket path (K > 4096: one launch per solve, merge by the last workgroup) overlaps its launches as well
    h->ticket_det = !h->slow_path && !p.slip_on && !h->pipelined && !(cfg->flags & BN_FLAG_NO_PIPELINE) && p.nblk <= 1024 &&
                    bn::finish_lds_bytes(p) + 256 <= bn::rollout_lds_bytes(p);
    h->ticket_overlap = (h->ticket_det || (!(cfg->flags & BN_FLAG_NO_PIPELINE) && bn::sampled_fused(p))) && !(cfg->flags & BN_FLAG_NO_OVERLAP) &&
                        !exp_env("BN_NO_TICKET_OVERLAP");
    h->may_overlap = (h->lat_kernel || h->role_overlap || h->ticket_overlap) && !(cfg->flags & BN_FLAG_NO_OVERLAP);
    if (h->may_overlap) {
        // Two launches in flight.  Measured with three (role kernel, 64 instances): 23.3 instead of 22.6 us per launch; with
        // four the launches starve each other of slots (waits expire).  The slot / buffer arithmetic of create holds for up to kMaxStreams.
        h->n_streams = 2;
        if (const char *e = exp_env("BN_OVERLAP_STREAMS")) h->n_streams = std::min(std::max(std::atoi(e), 2), kMaxStreams);   // experiments
        h->has_alt = true;
        // the journal's state snapshots: only a handle that can overlap ever journals (up to 16 MB per handle otherwise,
        // times the planners of a K-sharded or per-instance set-up).  At most 16 MB; B <= 341 get the journal's own 4096 entries.
        h->snap_cap = std::max<size_t>(64, std::min<size_t>(4096, ((size_t)16 << 20) / ((size_t)p.B * 12)));
    }
    h->has_slip_std = p.slip_on != 0;
    // K > 4096 (ticket_det): too many partials for every workgroup to re-merge; the last workgroup of a launch merges them
    h->has_ticket_buffers = p.slip_on || h->ticket_det;
    h->ticket_mode = p.slip_on ? !h->slow_path && !(cfg->flags & BN_FLAG_NO_PIPELINE) && bn::sampled_fused(p) : h->ticket_det;

    const size_t B = p.B, K = p.K, T = p.T, G = p.G, X = B * (T + 1) * 3 * (size_t)p.Kp * 4, U = B * T * 2 * (size_t)p.Kp * 4;
    uint64_t *bytes = h->buffer_bytes;
    bytes[BN_BUF_STATES] = X;
    bytes[BN_BUF_STATES_ALT] = h->has_alt && h->has_X ? X : 0;
    bytes[BN_BUF_CONTROLS] = h->has_U ? U : 0;
    bytes[BN_BUF_CONTROLS_ALT] = h->has_alt && h->has_U ? U : 0;
    bytes[BN_BUF_WEIGHTS] = bytes[BN_BUF_COSTS] = B * K * 4;
    bytes[BN_BUF_USTAR] = bytes[BN_BUF_MEAN] = B * T * 2 * 4;
    bytes[BN_BUF_XSTAR] = B * (T + 1) * 3 * 4;
    bytes[BN_BUF_USTAR_XSTAR] = bytes[BN_BUF_USTAR] + bytes[BN_BUF_XSTAR];   // U* then X* in ONE block: a caller copies both at once
    bytes[BN_BUF_MAP] = (size_t)h->n_maps * G * G * 4;
    bytes[BN_BUF_GOAL] = B * 2 * 4;
    h->nblk = p.nblk; h->Kp = p.Kp; h->pow2 = p.pow2; h->inv_lambda = p.inv_lambda; h->reach = p.reach; h->WN = p.WN; h->lds_park = p.lds_park;
    h->ref_order = p.ref_order; h->wrap_near = p.wrap_near; h->regen_steps = p.regen_steps; h->park_steps = p.park_steps; h->xs = p.xs;
    h->map_stride = p.map_stride; h->slip_on = p.slip_on;
    *out = plan;
    return BN_OK;
}

}  // namespace host
}  // namespace bn

using namespace bn::host;

extern "C" int bn_mppi_debug_plan(const bn_mppi_config *cfg, int32_t n_cus, bn_mppi_plan_info *out)
{
    if (!cfg || !out) return fail(BN_ERR_INVALID, "null argument");
    if (out->struct_size != sizeof(bn_mppi_plan_info))
        return fail(BN_ERR_INVALID, "bn_mppi_plan_info.struct_size %u != %zu (ABI mismatch)", out->struct_size, sizeof(bn_mppi_plan_info));
    MppiPlan m{};
    if (int rc = plan_mppi(*cfg, n_cus, &m)) return rc;
    *out = m;                                          // (the bn_mppi_plan_info part of it)
    return BN_OK;
}
