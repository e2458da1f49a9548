// segtrain_handle.h -- training the U-Net terrain classifier: the argument blocks and launchers of
// csrc/segtrain_kernels.hip and the handle of csrc/segtrain_host.cpp.  The network's graph and the tile sizes are unet_graph.h's,
// the forward convolution unet_handle.h's, the gather and the staging constants unet_conv_tile.h's.  Private to csrc/.
#pragma once
#include "unet_handle.h"

namespace bn {

constexpr int kSegPitch = 66;                // floats per LDS row of backward-weight: the 16 x 4 fragment read is conflict-free
constexpr int kSegTargetGroups = 512;        // backward-weight splits its pixel axis until about this many workgroups run ...
constexpr int kSegMaxChunks = 64;            // ... into at most this many partial sums per output element
constexpr double kSegBnEps = 1e-5, kSegBnMomentum = 0.1;

// The split rule of backward-weight, a function of the shape only: `chunks` partial sums of `stages` 64-pixel stages each.
struct SegSplit { int chunks, stages; };
inline SegSplit seg_split(int64_t npix, int cout, int k)
{
    const int64_t total = (npix + kUnetTile - 1) / kUnetTile;
    const int64_t tiles = (int64_t)((cout + kUnetTile - 1) / kUnetTile) * ((k + kUnetTile - 1) / kUnetTile);
    int64_t want = kSegTargetGroups / tiles;
    if (want < 1) want = 1;
    if (want > kSegMaxChunks) want = kSegMaxChunks;
    if (want > total) want = total;
    const int64_t stages = (total + want - 1) / want;
    return SegSplit{(int)((total + stages - 1) / stages), (int)stages};
}

// One convolution's geometry as the two gradient kernels read it.  The forward's (virtual) input is a (ca channels, optionally 2x
// nearest-upsampled) ++ b (cb channels) of hin x win; dy is (num_maps, cout, hout, wout).
struct SegConvGrad {
    const float *a, *b, *dy;
    const float *wt;                         // backward-data: the flipped weight [kpad][cinpad], k = co ks^2 + (ks-1-ky) ks + (ks-1-kx)
    const float *residual;                   // backward-data: what already sits in the destination, or nullptr
    float *out;                              // backward-weight: partial[chunk][cout][k]; backward-data: (num_maps, cin, hin, win)
    int32_t num_maps, ca, cb, hin, win, hout, wout, cout, k, kpad, cinpad, stride, pad, upsample, chunks, stages;
};

// launchers (segtrain_kernels.hip); every one enqueues on `stream` and returns hipGetLastError()
hipError_t seg_launch_wgrad(hipStream_t s, int ksize, const SegConvGrad &g);
hipError_t seg_launch_wgrad_reduce(hipStream_t s, const float *partial, float *dw, int64_t n, int chunks);
hipError_t seg_launch_dgrad_strided(hipStream_t s, int ksize, const SegConvGrad &g);
hipError_t seg_launch_flip(hipStream_t s, const float *w, float *wt, float *zero_bias, int cout, int cin, int ksize, int kpad, int cinpad);
hipError_t seg_launch_split(hipStream_t s, const float *dcat, float *da, float *dskip, int num_maps, int ca, int cb, int h, int w, int upsample,
                            int accumulate);
hipError_t seg_launch_bias_grad(hipStream_t s, const float *dy, float *db, int num_maps, int channels, int64_t cells);
hipError_t seg_launch_bn_forward(hipStream_t s, const float *x, const float *gamma, const float *beta, const float *residual, int relu,
                                 float *running_mean, float *running_var, float *y, double *stats, int num_maps, int channels, int64_t cells);
hipError_t seg_launch_bn_backward(hipStream_t s, const float *dy, const float *y, const float *x, const double *stats, const float *gamma, int relu,
                                  float *dx, float *dres, float *dgamma, float *dbeta, double *sums, int num_maps, int channels, int64_t cells);
hipError_t seg_launch_maxpool_backward(hipStream_t s, const float *x, const float *gout, float *gin, int64_t planes, int hin, int win, int accumulate);
hipError_t seg_launch_cross_entropy(hipStream_t s, const float *logits, const int64_t *targets, float *dlogits, double *terms, float *loss,
                                    int num_maps, int classes, int64_t cells);
hipError_t seg_launch_adam(hipStream_t s, float *p, const float *g, float *m, float *v, int64_t n, double lr, double beta1, double beta2, double eps,
                           double weight_decay, double correction1, double correction2_sqrt);

}  // namespace bn

// Device layout of the parameters: the trainable ones first, per convolution of the table its weight, then gamma and beta (the head:
// its bias); behind them the running statistics, per convolution mean then variance.  Gradients, m and v cover the trainable part.
struct bn_segtrain {
    int device = 0, classes = 0;
    int64_t steps = 0, trainable = 0, stats = 0;
    std::vector<bn::UnetConvDesc> layers;
    std::vector<size_t> weight_at, stats_at, wt_at;      // floats: into params (weight; gamma = + cout K), into params (mean), into wt
    bn::DeviceBuffers bufs;
    float *params = nullptr, *grads = nullptr, *m = nullptr, *v = nullptr, *wt = nullptr;
};
