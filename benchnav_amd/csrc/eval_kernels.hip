// eval_kernels.hip -- the model-evaluation stage on the device: how good are the trained models, measured on
// arrays that already sit on the device.  Three reductions over M maps of `cells` cells, each one pass:
//
//   confusion   (true class, predicted class) counts per map;
//   slip        per (true class, slope bin) sums of the predicted N(mu, sigma^2) against the latent N(m, s^2) and an observation y;
//   risk        per (risk setting, true class) counts of y above the risk map, and the 2 x 2 table of (believed stuck, actually stuck).
//
// Every count is an integer: LDS counters per workgroup, ONE 64-bit integer flush per workgroup, exact in any order.  The slip
// stage's float64 sums follow a FIXED order that is a function of the cell index and the map index alone (tests/evaluate_spec.py
// restates it operation for operation): a map is cut into slabs of BN_EVAL_SLAB_CELLS cells; one wave owns a slab and walks it in
// steps of 64 consecutive cells; per step and per group present in it, the 64 lanes' values (a lane that is no member holds +0.0)
// are reduced by the xor butterfly 32, 16, 8, 4, 2, 1 and the result is added to the wave's LDS table; the slab tables go to a
// workspace with plain stores; a second kernel adds a map's slabs in slab order, a third the maps in map order onto the caller's
// running total.  No float atomic anywhere, and neither M, the split of the maps over calls nor the grid enters the order.
#include "../../include/benchnav_mppi.h"
#include "bn_device_math.h"
#include "bn_host.h"

#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <string>

namespace bn {
namespace {

constexpr int kWave = 64;
constexpr int kCountThreads = 256;                     // the two counting kernels: four waves share one LDS table
constexpr int kSlab = BN_EVAL_SLAB_CELLS;
constexpr int kSums = BN_EVAL_SLIP_SUMS;
constexpr int kRiskCounts = BN_EVAL_RISK_COUNTS;
constexpr double kTwoPiF64 = 6.283185307179586;        // float64(2 pi), the spec's constant

typedef unsigned long long u64;

extern __shared__ __attribute__((aligned(16))) char eval_smem[];

// workgroup `bid` of a (slabs x maps) launch, flattened: grid.y stops at 65535 maps
struct Slab {
    int64_t map, base, end;
    __device__ Slab(int64_t bid, int64_t nslabs, int64_t cells)
    {
        map = bid / nslabs;
        base = (bid - map * nslabs) * kSlab;
        end = base + kSlab < cells ? base + kSlab : cells;
    }
};

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e+38f; }      // false for NaN and +-inf

// ---- a. confusion --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCountThreads) void confusion_kernel(const int32_t *__restrict__ truth, const int32_t *__restrict__ pred,
                                                                  int64_t cells, int64_t nslabs, int C, int64_t *__restrict__ table,
                                                                  int64_t *__restrict__ ignored)
{
    uint32_t *lds = (uint32_t *)eval_smem;             // C * C counters and the ignored one
    const int n = C * C + 1;
    for (int e = threadIdx.x; e < n; e += kCountThreads) lds[e] = 0u;
    __syncthreads();
    const Slab s(blockIdx.x, nslabs, cells);
    const int32_t *t = truth + s.map * cells, *p = pred + s.map * cells;
    for (int64_t cell = s.base + threadIdx.x; cell < s.end; cell += kCountThreads) {
        const int a = t[cell], b = p[cell];
        const bool ok = a >= 0 && a < C && b >= 0 && b < C;
        atomicAdd(&lds[ok ? a * C + b : C * C], 1u);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < n; e += kCountThreads) {
        const uint32_t v = lds[e];
        if (v) atomicAdd((u64 *)(e < C * C ? table + s.map * (C * C) + e : ignored + s.map), (u64)v);
    }
}

// ---- b. slip -------------------------------------------------------------------------------------------------------------------
struct SlipIn {
    const float *mu, *sigma, *m, *s, *phi, *y;         // y may be null
    const int32_t *cls;
};

__device__ __forceinline__ double wave_tree(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, kWave);
    return v;
}

// one wave per workgroup: the wave's table is the workgroup's, and only lane 0 touches it between the two barriers
__global__ __launch_bounds__(kWave) void slip_kernel(SlipIn in, int64_t cells, int64_t nslabs, int C, int NB, double max_slope,
                                                     double *__restrict__ slab_sums, int64_t *__restrict__ counts,
                                                     int64_t *__restrict__ invalid)
{
    const int groups = C * NB, lane = threadIdx.x;
    double *T = (double *)eval_smem;                               // (groups, kSums)
    uint32_t *N = (uint32_t *)(eval_smem + (size_t)groups * kSums * sizeof(double));   // (groups, 2): count, covered
    for (int e = lane; e < groups * kSums; e += kWave) T[e] = 0.0;
    for (int e = lane; e < groups * 2; e += kWave) N[e] = 0u;
    __syncthreads();
    const Slab sl(blockIdx.x, nslabs, cells);
    const size_t off = (size_t)sl.map * (size_t)cells;
    const int nk = in.y ? kSums : kSums - 2;
    uint32_t bad = 0;
    for (int64_t c0 = sl.base; c0 < sl.end; c0 += kWave) {
        const int64_t cell = c0 + lane;
        int g = -1;
        bool covered = false;
        double v[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (cell < sl.end) {
            const float fmu = in.mu[off + cell], fsg = in.sigma[off + cell], fm = in.m[off + cell], fs = in.s[off + cell];
            const float fphi = in.phi[off + cell], fy = in.y ? in.y[off + cell] : 0.0f;
            const int c = in.cls[off + cell];
            const bool ok = c >= 0 && c < C && finite_f(fphi) && finite_f(fmu) && finite_f(fsg) && finite_f(fm) && finite_f(fs) && finite_f(fy) &&
                            fsg > 0.0f && fs > 0.0f;
            if (ok) {
                const double t = ((double)fphi * (double)NB) / max_slope;
                const int j = t < 0.0 ? 0 : (t >= (double)NB ? NB - 1 : (int)t);
                g = c * NB + j;
                const double mu = fmu, sg = fsg, m = fm, s = fs;
                const double d = mu - m, two_var = (2.0 * sg) * sg;
                v[0] = d;
                v[1] = fabs(d);
                v[2] = d * d;
                v[3] = sg;
                v[4] = s;
                v[5] = (log(sg / s) + (s * s + d * d) / two_var) - 0.5;
                if (in.y) {
                    const double e = (double)fy - mu, z = e / sg;
                    v[6] = 0.5 * log(kTwoPiF64 * (sg * sg)) + (e * e) / two_var;
                    v[7] = z * z;
                    covered = fabs(e) <= 2.0 * sg;
                }
            }
        }
        bad += (uint32_t)__popcll(__ballot(cell < sl.end && g < 0));
        u64 todo = __ballot(g >= 0);
        while (todo) {                                             // wave-uniform: one turn per group present in these 64 cells
            const int gs = __shfl(g, __ffsll((long long)todo) - 1, kWave);
            const bool member = g == gs;
            const u64 mask = __ballot(member);
            const uint32_t n_cov = (uint32_t)__popcll(__ballot(member && covered));
#pragma unroll
            for (int k = 0; k < kSums; ++k) {
                if (k < nk) {                                      // without y the last two sums stay 0
                    const double r = wave_tree(member ? v[k] : 0.0);
                    if (lane == 0) T[gs * kSums + k] = T[gs * kSums + k] + r;
                }
            }
            if (lane == 0) {
                N[gs * 2 + 0] += (uint32_t)__popcll(mask);
                N[gs * 2 + 1] += n_cov;
            }
            todo &= ~mask;
        }
    }
    __syncthreads();
    double *out = slab_sums + (size_t)blockIdx.x * (size_t)(groups * kSums);      // blockIdx.x = map * nslabs + slab
    for (int e = lane; e < groups * kSums; e += kWave) out[e] = T[e];
    for (int e = lane; e < groups * 2; e += kWave) {
        const uint32_t n = N[e];
        if (n) atomicAdd((u64 *)(counts + sl.map * (groups * 2) + e), (u64)n);
    }
    if (lane == 0 && bad) atomicAdd((u64 *)(invalid + sl.map), (u64)bad);
}

// a map's table: its slabs' tables added in slab order, one thread per entry
__global__ __launch_bounds__(kCountThreads) void slip_maps_kernel(const double *__restrict__ slab_sums, int64_t nslabs, int E, int64_t blocks_per_map,
                                                                  double *__restrict__ sums)
{
    const int64_t map = blockIdx.x / blocks_per_map;
    const int e = (int)(blockIdx.x - map * blocks_per_map) * kCountThreads + threadIdx.x;
    if (e >= E) return;
    const double *w = slab_sums + (size_t)map * (size_t)nslabs * E + e;
    double p = 0.0;
    for (int64_t s = 0; s < nslabs; ++s) p = p + w[(size_t)s * E];
    sums[(size_t)map * E + e] = p;
}

// the running total: the maps' tables added onto it in map order
__global__ __launch_bounds__(kCountThreads) void slip_total_kernel(const double *__restrict__ sums, int M, int E, double *__restrict__ total)
{
    const int e = blockIdx.x * kCountThreads + threadIdx.x;
    if (e >= E) return;
    double t = total[e];
    for (int m = 0; m < M; ++m) t = t + sums[(size_t)m * E + e];
    total[e] = t;
}

// ---- c. risk -------------------------------------------------------------------------------------------------------------------
// the environment step's rule (mppi_env_step.h: trav = 1 - clamp(slip, 0, 1); bn_mppi_env_collision_check: trav <= threshold), float32
__device__ __forceinline__ bool stuck_f32(float slip, float thr) { return 1.0f - clampf(slip, 0.0f, 1.0f) <= thr; }

__global__ __launch_bounds__(kCountThreads) void risk_kernel(const float *__restrict__ risk, const float *__restrict__ slips,
                                                             const int32_t *__restrict__ cls, int S, int M, int64_t cells, int64_t nslabs,
                                                             int C, float thr, int64_t *__restrict__ counts, int64_t *__restrict__ invalid)
{
    uint32_t *lds = (uint32_t *)eval_smem;             // (S, C, kRiskCounts) counters, then S invalid ones
    const int per_setting = C * kRiskCounts, n = S * per_setting;
    for (int e = threadIdx.x; e < n + S; e += kCountThreads) lds[e] = 0u;
    __syncthreads();
    const Slab s(blockIdx.x, nslabs, cells);
    const size_t off = (size_t)s.map * (size_t)cells;
    for (int64_t cell = s.base + threadIdx.x; cell < s.end; cell += kCountThreads) {
        const float y = slips[off + cell];             // read once for all S settings
        const int c = cls[off + cell];
        const bool cell_ok = c >= 0 && c < C && finite_f(y);
        const int actual = stuck_f32(y, thr) ? 1 : 0;
        for (int k = 0; k < S; ++k) {
            const float r = risk[((size_t)k * M + (size_t)s.map) * (size_t)cells + cell];
            if (!cell_ok || !finite_f(r)) {
                atomicAdd(&lds[n + k], 1u);
                continue;
            }
            uint32_t *row = lds + k * per_setting + c * kRiskCounts;
            if (y > r) atomicAdd(&row[0], 1u);
            atomicAdd(&row[1 + 2 * (stuck_f32(r, thr) ? 1 : 0) + actual], 1u);
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < n + S; e += kCountThreads) {
        const uint32_t v = lds[e];
        if (v) atomicAdd((u64 *)(e < n ? counts + s.map * n + e : invalid + s.map * S + (e - n)), (u64)v);
    }
}

thread_local std::string g_eval_error;

int eval_fail(int code, const std::string &msg)
{
    g_eval_error = msg;
    return code;
}

// the checks every entry point shares; nslabs * M workgroups must fit one grid dimension
int check_maps(int32_t M, int64_t cells, int32_t C, int64_t *nslabs)
{
    if (M < 1) return eval_fail(BN_ERR_INVALID, "num_maps must be >= 1");
    if (cells < 1) return eval_fail(BN_ERR_INVALID, "cells must be >= 1");
    if (C < 1 || C > BN_EVAL_MAX_CLASSES) return eval_fail(BN_ERR_INVALID, "num_classes must be in [1, 64]");
    *nslabs = (cells - 1) / kSlab + 1;                  // cells >= 1: no overflow near INT64_MAX
    if (*nslabs > (int64_t)INT32_MAX / M) return eval_fail(BN_ERR_INVALID, "num_maps * cells is out of range");
    return BN_OK;
}

// ... and the slip stage's second launch, ceil(C * NB * kSums / kCountThreads) workgroups per map, one too
int check_bins(int32_t M, int32_t C, int32_t NB)
{
    if (NB < 1 || NB > BN_EVAL_MAX_BINS) return eval_fail(BN_ERR_INVALID, "num_bins must be in [1, 64]");
    if (C * NB > BN_EVAL_MAX_GROUPS) return eval_fail(BN_ERR_INVALID, "num_classes * num_bins must be <= 512");
    const int64_t blocks_per_map = (C * NB * kSums + kCountThreads - 1) / kCountThreads;
    if (blocks_per_map > (int64_t)INT32_MAX / M) return eval_fail(BN_ERR_INVALID, "num_maps * num_classes * num_bins is out of range");
    return BN_OK;
}

}  // namespace
}  // namespace bn

extern "C" {

const char *bn_eval_last_error(void) { return bn::g_eval_error.c_str(); }

int bn_eval_confusion_async(int32_t device_id, void *stream, const int32_t *true_classes_device, const int32_t *pred_classes_device,
                            int32_t num_maps, int64_t cells, int32_t num_classes, int64_t *table_device, int64_t *ignored_device)
{
    using bn::eval_fail;
    if (!true_classes_device || !pred_classes_device) return eval_fail(BN_ERR_INVALID, "null argument");
    if (!table_device || !ignored_device) return eval_fail(BN_ERR_INVALID, "null output");
    int64_t nslabs = 0;
    if (int rc = bn::check_maps(num_maps, cells, num_classes, &nslabs)) return rc;
    if (int rc = bn::open_device(device_id, eval_fail)) return rc;
    BN_ON_DEVICE(eval_fail, device_id);
    hipStream_t st = (hipStream_t)stream;
    const size_t C2 = (size_t)num_classes * num_classes;
    BN_HIP_OR(eval_fail, hipMemsetAsync(table_device, 0, (size_t)num_maps * C2 * sizeof(int64_t), st));
    BN_HIP_OR(eval_fail, hipMemsetAsync(ignored_device, 0, (size_t)num_maps * sizeof(int64_t), st));
    bn::confusion_kernel<<<(unsigned)(nslabs * num_maps), bn::kCountThreads, (C2 + 1) * sizeof(uint32_t), st>>>(
        true_classes_device, pred_classes_device, cells, nslabs, num_classes, table_device, ignored_device);
    BN_HIP_OR(eval_fail, hipGetLastError());
    return BN_OK;
}

size_t bn_eval_slip_workspace_bytes(int32_t num_maps, int64_t cells, int32_t num_classes, int32_t num_bins)
{
    int64_t nslabs = 0;
    if (bn::check_maps(num_maps, cells, num_classes, &nslabs) || bn::check_bins(num_maps, num_classes, num_bins)) return 0;
    return (size_t)num_maps * (size_t)nslabs * (size_t)(num_classes * num_bins) * bn::kSums * sizeof(double);
}

int bn_eval_slip_async(int32_t device_id, void *stream, const float *mean_device, const float *std_device, const float *latent_mean_device,
                       const float *latent_std_device, const float *slopes_device, const int32_t *classes_device, const float *slips_device,
                       int32_t num_maps, int64_t cells, int32_t num_classes, int32_t num_bins, double max_slope, double *sums_device,
                       int64_t *counts_device, int64_t *invalid_device, double *total_device, void *workspace_device, size_t workspace_bytes)
{
    using bn::eval_fail;
    if (!mean_device || !std_device || !latent_mean_device || !latent_std_device || !slopes_device || !classes_device)
        return eval_fail(BN_ERR_INVALID, "null argument");
    if (!sums_device || !counts_device || !invalid_device) return eval_fail(BN_ERR_INVALID, "null output");
    int64_t nslabs = 0;
    if (int rc = bn::check_maps(num_maps, cells, num_classes, &nslabs)) return rc;
    if (int rc = bn::check_bins(num_maps, num_classes, num_bins)) return rc;
    if (!(max_slope > 0.0) || !std::isfinite(max_slope)) return eval_fail(BN_ERR_INVALID, "max_slope must be > 0 and finite");
    const size_t need = bn_eval_slip_workspace_bytes(num_maps, cells, num_classes, num_bins);
    if (!workspace_device || workspace_bytes < need) return eval_fail(BN_ERR_INVALID, "workspace too small (bn_eval_slip_workspace_bytes)");
    if (int rc = bn::open_device(device_id, eval_fail)) return rc;
    BN_ON_DEVICE(eval_fail, device_id);
    hipStream_t st = (hipStream_t)stream;
    const int groups = num_classes * num_bins, E = groups * bn::kSums;
    BN_HIP_OR(eval_fail, hipMemsetAsync(counts_device, 0, (size_t)num_maps * groups * 2 * sizeof(int64_t), st));
    BN_HIP_OR(eval_fail, hipMemsetAsync(invalid_device, 0, (size_t)num_maps * sizeof(int64_t), st));
    const bn::SlipIn in{mean_device, std_device, latent_mean_device, latent_std_device, slopes_device, slips_device, classes_device};
    const size_t lds = (size_t)E * sizeof(double) + (size_t)groups * 2 * sizeof(uint32_t);
    bn::slip_kernel<<<(unsigned)(nslabs * num_maps), bn::kWave, lds, st>>>(in, cells, nslabs, num_classes, num_bins, max_slope,
                                                                           (double *)workspace_device, counts_device, invalid_device);
    BN_HIP_OR(eval_fail, hipGetLastError());
    const int64_t blocks_per_map = (E + bn::kCountThreads - 1) / bn::kCountThreads;
    bn::slip_maps_kernel<<<(unsigned)(blocks_per_map * num_maps), bn::kCountThreads, 0, st>>>((const double *)workspace_device, nslabs, E,
                                                                                              blocks_per_map, sums_device);
    BN_HIP_OR(eval_fail, hipGetLastError());
    if (total_device) {
        bn::slip_total_kernel<<<(unsigned)blocks_per_map, bn::kCountThreads, 0, st>>>(sums_device, num_maps, E, total_device);
        BN_HIP_OR(eval_fail, hipGetLastError());
    }
    return BN_OK;
}

int bn_eval_risk_async(int32_t device_id, void *stream, const float *risk_device, const float *slips_device, const int32_t *classes_device,
                       int32_t num_settings, int32_t num_maps, int64_t cells, int32_t num_classes, float stuck_threshold,
                       int64_t *counts_device, int64_t *invalid_device)
{
    using bn::eval_fail;
    if (!risk_device || !slips_device || !classes_device) return eval_fail(BN_ERR_INVALID, "null argument");
    if (!counts_device || !invalid_device) return eval_fail(BN_ERR_INVALID, "null output");
    if (num_settings < 1 || num_settings > BN_RISK_MAX_SETTINGS) return eval_fail(BN_ERR_INVALID, "num_settings must be in [1, 16]");
    int64_t nslabs = 0;
    if (int rc = bn::check_maps(num_maps, cells, num_classes, &nslabs)) return rc;
    if (!std::isfinite(stuck_threshold)) return eval_fail(BN_ERR_INVALID, "stuck_threshold must be finite");
    if (int rc = bn::open_device(device_id, eval_fail)) return rc;
    BN_ON_DEVICE(eval_fail, device_id);
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)num_settings * num_classes * bn::kRiskCounts;
    BN_HIP_OR(eval_fail, hipMemsetAsync(counts_device, 0, (size_t)num_maps * n * sizeof(int64_t), st));
    BN_HIP_OR(eval_fail, hipMemsetAsync(invalid_device, 0, (size_t)num_maps * num_settings * sizeof(int64_t), st));
    bn::risk_kernel<<<(unsigned)(nslabs * num_maps), bn::kCountThreads, (n + num_settings) * sizeof(uint32_t), st>>>(
        risk_device, slips_device, classes_device, num_settings, num_maps, cells, nslabs, num_classes, stuck_threshold, counts_device,
        invalid_device);
    BN_HIP_OR(eval_fail, hipGetLastError());
    return BN_OK;
}

}  // extern "C"
