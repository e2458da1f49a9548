// unet_conv_tile.h -- device code the U-Net's convolution kernels share (unet_kernels.hip, segtrain_kernels.hip): the staging
// constants of the 64 x 64 tile and the gather of the forward's virtual input.  unet_kernels.hip's head describes the tiling and
// the summation order.  Included by .hip files only.
#pragma once
#include <hip/hip_runtime.h>

#include "unet_graph.h"

namespace bn {
namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kPitch = 80;                   // floats per LDS row: 64 + 16
constexpr int kStage = 64;                   // k rows staged through LDS per main-loop step (the last step may hold fewer)
constexpr int kRows = kStage / 4;            // rows of each operand a thread stages: one column, every fourth row
constexpr int kSlabStages = 2;               // 2 stages of 64 k = one slab of 128

// One element of the (virtual) input matrix of convolution arguments p (UnetConvArgs or SegConvGrad): row k, this lane's pixel.
// k is the same for the 64 lanes of a wave (wave-uniform: a wave stages whole rows), so its split into channel and tap, the choice between
// the two tensors and the channel's offset run on the scalar unit; a lane adds its pixel's 32-bit offset inside the map (a map's
// tensor holds fewer than 2^31 elements).
template <int KS, typename Args>
__device__ __forceinline__ float unet_gather(const Args &p, int k, bool pixel_valid, const float *map_a, const float *map_b, int iy0, int ix0)
{
    const int ci = k / (KS * KS), tap = k - ci * (KS * KS), ky = tap / KS, kx = tap - ky * KS;
    const int iy = iy0 + ky, ix = ix0 + kx;
    if (!pixel_valid || k >= p.k || iy < 0 || iy >= p.hin || ix < 0 || ix >= p.win) return 0.0f;    // zero padding, the K tail
    if (ci < p.ca) {
        if (p.upsample) {
            const int ha = p.hin >> 1, wa = p.win >> 1;
            return map_a[ci * (ha * wa) + (iy >> 1) * wa + (ix >> 1)];
        }
        return map_a[ci * (p.hin * p.win) + iy * p.win + ix];
    }
    return map_b[(ci - p.ca) * (p.hin * p.win) + iy * p.win + ix];
}

}  // namespace
}  // namespace bn
