// dataset_kernels.hip -- the dataset stage's two device operations.
//
//  * the slip observations of SlipRegressionDataset.__getitem__ (reference src/data/terrain_dataset.py:124-133,
//    `distributions["latent_models"].sample()`) as a keyed Philox stream: cell i of map m (global index in the split) at epoch e
//    is draw i & 3 of block {i >> 2, m, e, 'OBSV'} under the key (lo(seed), hi(seed)), and slip = z * std + mean as a rounded
//    product and a rounded sum (Normal.sample's normal_().mul_(std).add_(mean); this file is built with -ffp-contract=off);
//  * RegressorTrainer.load_data (reference src/trainers/regressor_trainer.py:90-126): per terrain class the slopes and slips of
//    its cells, map after map in a visiting order, row-major inside a map, cut at `cap`.  Three launches: a per-map per-class
//    count, an exclusive scan per class over the maps in visiting order, and a scatter with one workgroup per map whose ranks
//    come from wave ballots and cross-wave offsets -- integers only, no atomics on the destination, so the order is the
//    reference's and two runs give the same bits whatever the launch geometry.
//
// No handle: raw device pointers, the caller's stream, the caller's workspace.  Errors: bn_dataset_last_error().
#include "../../include/benchnav_mppi.h"
#include "bn_device_math.h"
#include "bn_host.h"

#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>

namespace bn {
namespace {

constexpr int kDatasetThreads = 256;                 // 4 waves per workgroup
constexpr int kDatasetWaves = kDatasetThreads / 64;
constexpr int kDatasetMaxClasses = 64;               // the per-class tables live in LDS
constexpr uint32_t kObservationWord = 0x4F425356u;   // 'OBSV'
constexpr int64_t kMaxGridBlocks = 1 << 20;          // maps beyond this are reached by the grid-stride loops

__device__ __forceinline__ void observation_block(uint64_t seed, uint32_t map, uint32_t epoch, uint32_t j, float z[4])
{
    const u32x4 r = philox4x32_10(u32x4{j, map, epoch, kObservationWord}, (uint32_t)seed, (uint32_t)(seed >> 32));
    box_muller(r.x, r.y, z[0], z[1]);
    box_muller(r.z, r.w, z[2], z[3]);
}

// Normal.sample(): normal_(0, 1).mul_(std).add_(mean) -- two roundings
__device__ __forceinline__ float observe(float z, float mean, float stdv) { return z * stdv + mean; }

// the observation of ONE cell, for the gather that draws only what it keeps: the same block, the same functions
__device__ __forceinline__ float observation_of_cell(uint64_t seed, uint32_t map, uint32_t epoch, int64_t cell, float mean, float stdv)
{
    float z[4];
    observation_block(seed, map, epoch, (uint32_t)(cell >> 2), z);
    const int s = (int)(cell & 3);
    const float zz = s == 0 ? z[0] : s == 1 ? z[1] : s == 2 ? z[2] : z[3];
    return observe(zz, mean, stdv);
}

// one thread per Philox block (four cells) of one map
__global__ __launch_bounds__(kDatasetThreads) void sample_slips_kernel(const float *__restrict__ mean, const float *__restrict__ stdv,
                                                                       const float *__restrict__ z_in, float *__restrict__ slips,
                                                                       int64_t num_maps, int64_t cells, int64_t blocks_per_map,
                                                                       int64_t first_map, uint64_t seed, uint32_t epoch)
{
    const int64_t total = num_maps * blocks_per_map;
    for (int64_t t = (int64_t)blockIdx.x * kDatasetThreads + threadIdx.x; t < total; t += (int64_t)gridDim.x * kDatasetThreads) {
        const int64_t m = t / blocks_per_map, j = t - m * blocks_per_map;
        const int64_t c0 = 4 * j, base = m * cells;
        float z[4];
        if (z_in) {
#pragma unroll
            for (int s = 0; s < 4; ++s) z[s] = (c0 + s < cells) ? z_in[base + c0 + s] : 0.0f;
        } else {
            observation_block(seed, (uint32_t)(first_map + m), epoch, (uint32_t)j, z);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (c0 + s < cells) slips[base + c0 + s] = observe(z[s], mean[base + c0 + s], stdv[base + c0 + s]);
    }
}

__device__ __forceinline__ int64_t visited_map(const int64_t *__restrict__ order, int64_t p, int64_t num_maps)
{
    const int64_t m = order ? order[p] : p;
    return (m >= 0 && m < num_maps) ? m : -1;           // an entry outside [0, M) names no map: nothing is read for it
}

// phase 1: counts[p, k] = cells of class k in the map visited at position p
__global__ __launch_bounds__(kDatasetThreads) void gather_count_kernel(const int32_t *__restrict__ classes, const int64_t *__restrict__ order,
                                                                       int32_t *__restrict__ counts, int64_t num_maps, int64_t cells, int C)
{
    __shared__ int hist[kDatasetMaxClasses];
    for (int64_t p = blockIdx.x; p < num_maps; p += gridDim.x) {
        for (int k = threadIdx.x; k < C; k += kDatasetThreads) hist[k] = 0;
        __syncthreads();
        const int64_t m = visited_map(order, p, num_maps);
        if (m >= 0) {
            const int32_t *row = classes + m * cells;
            for (int64_t i = threadIdx.x; i < cells; i += kDatasetThreads) {
                const int32_t c = row[i];
                if (c >= 0 && c < C) atomicAdd(&hist[c], 1);        // an integer sum: the same whatever the order
            }
        }
        __syncthreads();
        for (int k = threadIdx.x; k < C; k += kDatasetThreads) counts[p * C + k] = hist[k];
        __syncthreads();
    }
}

// phase 2: one workgroup per class; offsets[p, k] = sum of counts[q, k] over q < p, totals[k] the whole sum
__global__ __launch_bounds__(kDatasetThreads) void gather_scan_kernel(const int32_t *__restrict__ counts, int64_t *__restrict__ offsets,
                                                                      int64_t *__restrict__ totals, int32_t *__restrict__ kept,
                                                                      int64_t num_maps, int C, int cap)
{
    __shared__ int64_t part[kDatasetThreads];
    __shared__ int64_t carry_s;
    const int k = blockIdx.x, t = threadIdx.x;
    if (k >= C) return;
    if (t == 0) carry_s = 0;
    __syncthreads();
    for (int64_t base = 0; base < num_maps; base += kDatasetThreads) {
        const int64_t p = base + t;
        const int64_t own = p < num_maps ? (int64_t)counts[p * C + k] : 0;
        part[t] = own;
        __syncthreads();
        for (int step = 1; step < kDatasetThreads; step <<= 1) {          // inclusive scan of the chunk
            const int64_t add = t >= step ? part[t - step] : 0;
            __syncthreads();
            part[t] += add;
            __syncthreads();
        }
        const int64_t carry = carry_s;
        if (p < num_maps) offsets[p * C + k] = carry + part[t] - own;
        __syncthreads();
        if (t == kDatasetThreads - 1) carry_s = carry + part[t];
        __syncthreads();
    }
    if (t == 0) {
        totals[k] = carry_s;
        kept[k] = (int32_t)(carry_s < (int64_t)cap ? carry_s : (int64_t)cap);
    }
}

// phase 3: one workgroup per visited map writes the cells that land below the cap, in row-major order per class
__global__ __launch_bounds__(kDatasetThreads) void gather_scatter_kernel(const float *__restrict__ slopes, const float *__restrict__ slips,
                                                                         const float *__restrict__ mean, const float *__restrict__ stdv,
                                                                         const int32_t *__restrict__ classes, const int64_t *__restrict__ order,
                                                                         const int32_t *__restrict__ counts, const int64_t *__restrict__ offsets,
                                                                         float *__restrict__ x, float *__restrict__ y, int64_t num_maps,
                                                                         int64_t cells, int C, int cap, uint64_t seed, uint32_t epoch)
{
    __shared__ int64_t start[kDatasetMaxClasses];                 // where the map's first cell of class k goes
    __shared__ int have[kDatasetMaxClasses];                      // how many cells of class k the map holds
    __shared__ int done[kDatasetMaxClasses];                      // ... and how many the chunks so far held
    __shared__ int wave_count[kDatasetWaves][kDatasetMaxClasses];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint64_t lower = lane ? (~0ull >> (64 - lane)) : 0ull;  // the lanes below this one (wave64: 64-bit masks)
    for (int64_t p = blockIdx.x; p < num_maps; p += gridDim.x) {
        __syncthreads();                                          // the tables of the previous map are no longer read
        if (t < C) {
            start[t] = offsets[p * C + t];
            have[t] = counts[p * C + t];
            done[t] = 0;
        }
        __syncthreads();
        const int64_t m = visited_map(order, p, num_maps);
        if (m < 0) continue;                                      // uniform over the workgroup
        const int64_t row = m * cells;
        for (int64_t base = 0; base < cells; base += kDatasetThreads) {
            // anything left to write?  (every offset already at or past the cap, or every cell of the map seen: nothing)
            const int live = t < C && done[t] < have[t] && start[t] + done[t] < (int64_t)cap;
            if (!__syncthreads_or(live)) break;
            const int64_t i = base + t;
            int32_t c = i < cells ? classes[row + i] : -1;
            if (c < 0 || c >= C) c = -1;
            int rank = 0;
            for (int k = 0; k < C; ++k) {
                const uint64_t mask = __ballot(c == k);
                if (c == k) rank = __popcll(mask & lower);
                if (lane == 0) wave_count[wave][k] = __popcll(mask);
            }
            __syncthreads();
            if (c >= 0) {
                int before = done[c];
                for (int w = 0; w < wave; ++w) before += wave_count[w][c];
                const int64_t dest = start[c] + before + rank;
                if (dest < (int64_t)cap) {
                    const int64_t at = (int64_t)c * cap + dest;
                    x[at] = slopes[row + i];
                    y[at] = slips ? slips[row + i] : observation_of_cell(seed, (uint32_t)m, epoch, i, mean[row + i], stdv[row + i]);
                }
            }
            __syncthreads();
            if (t < C) {
                int add = 0;
                for (int w = 0; w < kDatasetWaves; ++w) add += wave_count[w][t];
                done[t] += add;
            }
            // the __syncthreads_or at the head of the next chunk orders this update before its readers
        }
    }
}

thread_local std::string g_dataset_error;

int dataset_fail(int code, const std::string &msg)
{
    g_dataset_error = msg;
    return code;
}

constexpr int64_t kMaxMaps = (int64_t)1 << 32;        // the map index is one 32-bit counter word
constexpr int64_t kMaxCells = (int64_t)1 << 31;

int grid_for(int64_t work_items)
{
    const int64_t blocks = work_items < kMaxGridBlocks ? work_items : kMaxGridBlocks;
    return (int)(blocks < 1 ? 1 : blocks);
}

}  // namespace
}  // namespace bn

extern "C" {

const char *bn_dataset_last_error(void) { return bn::g_dataset_error.c_str(); }

int bn_dataset_sample_slips_async(int32_t device_id, void *stream, const float *mean_device, const float *std_device, const float *z_device,
                                  int64_t num_maps, int64_t cells, int64_t first_map, uint64_t seed, uint32_t epoch, float *slips_device)
{
    using bn::dataset_fail;
    if (!mean_device || !std_device || !slips_device) return dataset_fail(BN_ERR_INVALID, "null argument");
    if (num_maps < 1 || cells < 1 || cells >= bn::kMaxCells) return dataset_fail(BN_ERR_INVALID, "num_maps must be >= 1 and cells in [1, 2^31)");
    if (first_map < 0 || num_maps >= bn::kMaxMaps || first_map >= bn::kMaxMaps || first_map + num_maps > bn::kMaxMaps)
        return dataset_fail(BN_ERR_INVALID, "map indices must stay below 2^32");
    if (int rc = bn::open_device(device_id, dataset_fail)) return rc;
    BN_ON_DEVICE(dataset_fail, device_id);
    const int64_t blocks_per_map = (cells + 3) / 4;
    const int64_t threads = num_maps * blocks_per_map;
    bn::sample_slips_kernel<<<bn::grid_for((threads + bn::kDatasetThreads - 1) / bn::kDatasetThreads), bn::kDatasetThreads, 0, (hipStream_t)stream>>>(
        mean_device, std_device, z_device, slips_device, num_maps, cells, blocks_per_map, first_map, seed, epoch);
    BN_HIP_OR(dataset_fail, hipGetLastError());
    return BN_OK;
}

size_t bn_dataset_gather_workspace_bytes(int64_t num_maps, int32_t num_classes)
{
    if (num_maps < 1 || num_maps >= bn::kMaxMaps || num_classes < 1 || num_classes > bn::kDatasetMaxClasses) return 0;
    return (size_t)num_maps * (size_t)num_classes * (sizeof(int64_t) + sizeof(int32_t));
}

int bn_dataset_gather_async(int32_t device_id, void *stream, const float *slopes_device, const float *slips_device, const float *mean_device,
                            const float *std_device, const int32_t *classes_device, const int64_t *order_device, int64_t num_maps, int64_t cells,
                            int32_t num_classes, int32_t cap, uint64_t seed, uint32_t epoch, float *x_device, float *y_device,
                            int32_t *counts_device, int64_t *totals_device, void *workspace_device, size_t workspace_bytes)
{
    using bn::dataset_fail;
    if (!slopes_device || !classes_device || !x_device || !y_device || !counts_device || !totals_device || !workspace_device)
        return dataset_fail(BN_ERR_INVALID, "null argument");
    if (!slips_device && (!mean_device || !std_device))
        return dataset_fail(BN_ERR_INVALID, "null argument: without slips the observations are drawn from mean and std");
    if (num_classes < 1 || num_classes > bn::kDatasetMaxClasses) return dataset_fail(BN_ERR_INVALID, "num_classes must be in [1, 64]");
    if (cap < 1) return dataset_fail(BN_ERR_INVALID, "cap must be >= 1");
    if (num_maps < 1 || num_maps >= bn::kMaxMaps) return dataset_fail(BN_ERR_INVALID, "num_maps must be in [1, 2^32)");
    if (cells < 1 || cells >= bn::kMaxCells) return dataset_fail(BN_ERR_INVALID, "cells must be in [1, 2^31)");
    if (workspace_bytes < bn_dataset_gather_workspace_bytes(num_maps, num_classes)) return dataset_fail(BN_ERR_INVALID, "workspace too small");
    if (int rc = bn::open_device(device_id, dataset_fail)) return rc;
    BN_ON_DEVICE(dataset_fail, device_id);
    hipStream_t s = (hipStream_t)stream;
    int64_t *offsets = (int64_t *)workspace_device;                                   // (M, C), visiting position major
    int32_t *counts = (int32_t *)(offsets + num_maps * (int64_t)num_classes);         // (M, C)
    const int grid = bn::grid_for(num_maps);
    bn::gather_count_kernel<<<grid, bn::kDatasetThreads, 0, s>>>(classes_device, order_device, counts, num_maps, cells, num_classes);
    BN_HIP_OR(dataset_fail, hipGetLastError());
    bn::gather_scan_kernel<<<num_classes, bn::kDatasetThreads, 0, s>>>(counts, offsets, totals_device, counts_device, num_maps, num_classes, cap);
    BN_HIP_OR(dataset_fail, hipGetLastError());
    bn::gather_scatter_kernel<<<grid, bn::kDatasetThreads, 0, s>>>(slopes_device, slips_device, mean_device, std_device, classes_device, order_device,
                                                                   counts, offsets, x_device, y_device, num_maps, cells, num_classes, cap, seed, epoch);
    BN_HIP_OR(dataset_fail, hipGetLastError());
    return BN_OK;
}

}  // extern "C"
