// unet_handle.h -- the U-Net terrain classifier's layer table, its handle and the launchers of csrc/unet_kernels.hip, shared with
// the host file that drives them (unet_host.cpp).  Private to csrc/.
#pragma once
#include <cstdint>
#include <vector>

#include "bn_host.h"

namespace bn {

constexpr int kUnetMaxClasses = 32;
constexpr int kUnetTile = 64;                // the convolution's block tile: 64 output channels x 64 output pixels
constexpr int kUnetKStep = 16;               // the k rows of a convolution are padded to a multiple of this (four MFMA steps)
constexpr int kUnetMinSide = 32, kUnetMaxSide = 2048, kUnetMaxMaps = 4096;
constexpr int64_t kUnetMaxPixels = (int64_t)1 << 24;      // num_maps * H * W

inline int unet_round_up(int v, int m) { return (v + m - 1) / m * m; }

// one convolution of the network, in the order of the packed parameters (include/benchnav_mppi.h)
struct UnetConvDesc {
    int cin, cout, ksize, stride, pad;
    int K() const { return cin * ksize * ksize; }
    int kpad() const { return unet_round_up(K(), kUnetKStep); }
    int coutpad() const { return unet_round_up(cout, kUnetTile); }
    size_t host_floats() const { return (size_t)cout * K() + cout; }                // weights, then bias
    size_t device_floats() const { return (size_t)kpad() * coutpad() + coutpad(); }   // wt[kpad][coutpad], then bias[coutpad]
};

// indices into the table below
enum { kUnetStem = 0, kUnetLayer1 = 1, kUnetLayer2 = 5, kUnetLayer3 = 10, kUnetLayer4 = 15, kUnetDecoder = 20, kUnetHead = 30, kUnetConvs = 31 };

inline std::vector<UnetConvDesc> unet_layers(int classes)
{
    std::vector<UnetConvDesc> v;
    v.push_back({3, 64, 7, 2, 3});
    const int width[4] = {64, 128, 256, 512};
    int cin = 64;
    for (int l = 0; l < 4; ++l) {
        const int w = width[l], s = l ? 2 : 1;
        v.push_back({cin, w, 3, s, 1});                   // block 0: conv1, conv2, (downsample)
        v.push_back({w, w, 3, 1, 1});
        if (l) v.push_back({cin, w, 1, 2, 0});
        v.push_back({w, w, 3, 1, 1});                     // block 1: conv1, conv2
        v.push_back({w, w, 3, 1, 1});
        cin = w;
    }
    const int din[5] = {512, 256, 128, 64, 32}, dskip[5] = {256, 128, 64, 64, 0}, dout[5] = {256, 128, 64, 32, 16};
    for (int b = 0; b < 5; ++b) {
        v.push_back({din[b] + dskip[b], dout[b], 3, 1, 1});
        v.push_back({dout[b], dout[b], 3, 1, 1});
    }
    v.push_back({16, classes, 3, 1, 1});
    return v;
}

// One fused convolution as the kernel reads it.  The input is tensor a (ca channels), optionally 2x nearest-upsampled, followed
// along channels by tensor b (cb channels, may be 0); hin x win is the size of that (virtual) input.
struct UnetConvArgs {
    const float *a, *b;
    const float *wt, *bias;                  // wt[kpad][coutpad], bias[coutpad]
    const float *residual;                   // (num_maps, cout, hout, wout) or nullptr
    float *out;
    int32_t num_maps, ca, cb, hin, win, hout, wout, cout, coutpad, k, kpad, stride, pad, upsample, relu;
};

// launchers (unet_kernels.hip); every one enqueues on `stream` and returns hipGetLastError()
hipError_t unet_launch_conv(hipStream_t stream, int ksize, const UnetConvArgs &args);
hipError_t unet_launch_relayout(hipStream_t stream, const float *w, const float *bias, float *wt, float *bias_pad, int cout, int k, int kpad, int coutpad);
hipError_t unet_launch_maxpool(hipStream_t stream, const float *in, float *out, int64_t planes, int hin, int win, int hout, int wout);
hipError_t unet_launch_head(hipStream_t stream, const float *logits, float *probabilities, int32_t *classes, int num_maps, int num_classes, int64_t cells);

}  // namespace bn

struct bn_unet {
    int device = 0, classes = 0;
    std::vector<bn::UnetConvDesc> layers;
    std::vector<size_t> offset;              // of each layer's wt in `weights`, in floats; its bias follows at kpad * coutpad
    bn::DeviceBuffers bufs;
    float *weights = nullptr;
};
