// unet_handle.h -- the U-Net terrain classifier's handle, the convolution's argument block and the launchers of
// csrc/unet_kernels.hip, shared with the host file that drives them (unet_host.cpp).  The network itself -- the layer table, the
// nodes and their geometry -- is unet_graph.h's.  Private to csrc/.
#pragma once
#include "bn_host.h"
#include "unet_graph.h"

namespace bn {

constexpr int kUnetMinSide = 32, kUnetMaxSide = 2048, kUnetMaxMaps = 4096;
constexpr int64_t kUnetMaxPixels = (int64_t)1 << 24;      // num_maps * H * W

// One fused convolution as the kernel reads it.  The input is tensor a (ca channels), optionally 2x nearest-upsampled, followed
// along channels by tensor b (cb channels, may be 0); hin x win is the size of that (virtual) input.
struct UnetConvArgs {
    const float *a, *b;
    const float *wt, *bias;                  // wt[kpad][coutpad], bias[coutpad]
    const float *residual;                   // (num_maps, cout, hout, wout) or nullptr
    float *out;
    int32_t num_maps, ca, cb, hin, win, hout, wout, cout, coutpad, k, kpad, stride, pad, upsample, relu;
};

// the argument block of convolution d at geometry geo: a holds ca of d.cin channels, b the rest; the bias follows wt's kpad rows
inline UnetConvArgs unet_conv_args(const UnetConvDesc &d, const UnetGeo &geo, int num_maps, const float *a, int ca, const float *b, int upsample,
                                   const float *wt, const float *residual, int relu, float *out)
{
    UnetConvArgs g{};
    g.a = a; g.b = b; g.wt = wt; g.bias = wt + (size_t)d.kpad() * d.coutpad(); g.residual = residual; g.out = out;
    g.num_maps = num_maps; g.ca = ca; g.cb = d.cin - ca; g.hin = geo.hin; g.win = geo.win; g.hout = geo.hout; g.wout = geo.wout;
    g.cout = d.cout; g.coutpad = d.coutpad(); g.k = d.K(); g.kpad = d.kpad(); g.stride = d.stride; g.pad = d.pad;
    g.upsample = upsample; g.relu = relu;
    return g;
}

// The single-convolution entry points' range checks: nullptr, or why the arguments are refused.  The backward also needs
// pad <= ksize - 1 (its stride-1 data gradient is a convolution with pad ksize - 1 - pad).
inline const char *unet_conv_check(int ca, int cb, int cout, int ksize, int stride, int pad, int upsample, int num_maps, int hin, int win, bool backward)
{
    if (ca < 1 || cb < 0 || ca + cb > 4096 || cout < 1 || cout > 4096) return "ca must be >= 1, cb >= 0, and input and output channels in [1, 4096]";
    if (ksize != 1 && ksize != 3 && ksize != 7) return "ksize must be 1, 3 or 7";
    if (stride < 1 || stride > 2 || pad < 0 || pad > 3) return "stride must be 1 or 2 and pad in [0, 3]";
    if (backward && pad > ksize - 1) return "the backward needs pad <= ksize - 1";
    if (upsample != 0 && upsample != 1) return "upsample must be 0 or 1";
    if (num_maps < 1 || num_maps > kUnetMaxMaps || hin < 1 || hin > kUnetMaxSide || win < 1 || win > kUnetMaxSide)
        return "num_maps must be in [1, 4096] and the input sides in [1, 2048]";
    if (upsample && ((hin | win) & 1)) return "an upsampled input has even sides";
    if (hin + 2 * pad < ksize || win + 2 * pad < ksize) return "the kernel does not fit the padded input";
    const int64_t hout = (hin + 2 * pad - ksize) / stride + 1, wout = (win + 2 * pad - ksize) / stride + 1;
    if ((int64_t)num_maps * hin * win > kUnetMaxPixels || num_maps * hout * wout > kUnetMaxPixels) return "num_maps x pixels must be <= 2^24";
    if ((int64_t)num_maps * (ca + cb) * hin * win >= ((int64_t)1 << 31) || num_maps * cout * hout * wout >= ((int64_t)1 << 31))
        return "a tensor must hold fewer than 2^31 elements";
    return nullptr;
}

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
