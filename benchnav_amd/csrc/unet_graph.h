// unet_graph.h -- the U-Net terrain classifier described once: the table of its 31 convolutions in the order of the
// packed parameters, the table of its nodes in execution order, and every convolution's geometry for a map size.  Inference
// (unet_host.cpp) walks the nodes forwards; training (segtrain_host.cpp) walks them forwards, then in reverse.  Host code, private
// to csrc/.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace bn {

constexpr int kUnetMaxClasses = 32;
constexpr int kUnetTile = 64;                // the convolution's block tile: 64 output channels x 64 output pixels
constexpr int kUnetKStep = 16;               // the k rows of a convolution are padded to a multiple of this (four MFMA steps)

inline int unet_round_up(int v, int m) { return (v + m - 1) / m * m; }
inline size_t unet_align(size_t v) { return (v + 255) & ~(size_t)255; }       // workspace blocks start on multiples of 256 bytes

// one convolution of the network, in the order of the packed parameters (include/benchnav_mppi.h)
struct UnetConvDesc {
    int cin, cout, ksize, stride, pad;
    int K() const { return cin * ksize * ksize; }
    int kpad() const { return unet_round_up(K(), kUnetKStep); }
    int coutpad() const { return unet_round_up(cout, kUnetTile); }
    size_t host_floats() const { return (size_t)cout * K() + cout; }                // weights, then bias
    size_t device_floats() const { return (size_t)kpad() * coutpad() + coutpad(); }   // wt[kpad][coutpad], then bias[coutpad]
};

constexpr int kUnetHead = 30, kUnetConvs = 31;

inline std::vector<UnetConvDesc> unet_layers(int classes)
{
    std::vector<UnetConvDesc> v;
    v.reserve(kUnetConvs);
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

// A tensor of the graph is named by its slot: a convolution's index in the table above, or the max-pool's output.
constexpr int kUnetPool = kUnetConvs, kUnetSlots = kUnetConvs + 1, kUnetNodes = kUnetSlots, kUnetColors = -1, kUnetNone = -2;

// One node: out = relu?(conv_out(up2x?(in) ++ skip) + residual), or out = maxpool(in) where out is kUnetPool.  `reuse`: at inference
// the output overwrites that slot's buffer, which nothing reads any more (training keeps every activation).
struct UnetNode { int out, in, skip, upsample, residual, relu, reuse; };

// The nodes in execution order.  A layer's downsample stands before the convolution that shares its input: the two are independent,
// and training's backward -- this order reversed -- then adds into that input's gradient the decoder's skip gradient first, then
// block 0's conv1, then the downsample.  Float addition of three terms depends on that order.
inline const UnetNode *unet_nodes()
{
    constexpr int _ = kUnetNone, P = kUnetPool;
    static constexpr UnetNode nodes[kUnetNodes] = {
        // out, in, skip, upsample, residual, relu, reuse
        {0, kUnetColors, _, 0, _, 1, _},                                                                  // conv1 + bn1 + ReLU
        {P, 0, _, 0, _, 0, _},
        {1, P, _, 0, _, 1, _}, {2, 1, _, 0, P, 1, _}, {3, 2, _, 0, _, 1, 1}, {4, 3, _, 0, 2, 1, _},        // layer1
        {7, 4, _, 0, _, 0, _}, {5, 4, _, 0, _, 1, _}, {6, 5, _, 0, 7, 1, _}, {8, 6, _, 0, _, 1, 5}, {9, 8, _, 0, 6, 1, _},            // layer2
        {12, 9, _, 0, _, 0, _}, {10, 9, _, 0, _, 1, _}, {11, 10, _, 0, 12, 1, _}, {13, 11, _, 0, _, 1, 10}, {14, 13, _, 0, 11, 1, _},  // layer3
        {17, 14, _, 0, _, 0, _}, {15, 14, _, 0, _, 1, _}, {16, 15, _, 0, 17, 1, _}, {18, 16, _, 0, _, 1, 15}, {19, 18, _, 0, 16, 1, _},  // layer4
        {20, 19, 14, 1, _, 1, _}, {21, 20, _, 0, _, 1, _},                                                // the decoder's five blocks
        {22, 21, 9, 1, _, 1, _}, {23, 22, _, 0, _, 1, _},
        {24, 23, 4, 1, _, 1, _}, {25, 24, _, 0, _, 1, _},
        {26, 25, 0, 1, _, 1, _}, {27, 26, _, 0, _, 1, _},
        {28, 27, _, 1, _, 1, _}, {29, 28, _, 0, _, 1, _},
        {kUnetHead, 29, _, 0, _, 0, _},
    };
    return nodes;
}

// the slots bn_unet_feature_layout reports: the five encoder features, then the five decoder blocks' outputs
constexpr int kUnetFeatures[10] = {0, 4, 9, 14, 19, 21, 23, 25, 27, 29};

inline int unet_channels(const std::vector<UnetConvDesc> &layers, int slot)
{
    return slot == kUnetNone ? 0 : slot == kUnetColors ? layers[0].cin : layers[slot == kUnetPool ? 0 : slot].cout;
}

// Per slot the size of the node's (virtual) input -- its `in` tensor, upsampled where the node says so -- and of its output.
struct UnetGeo { int hin, win, hout, wout; };

inline std::vector<UnetGeo> unet_geometry(const std::vector<UnetConvDesc> &layers, int H, int W)
{
    std::vector<UnetGeo> g(kUnetSlots);
    const UnetNode *nodes = unet_nodes();
    const UnetConvDesc pool{0, 0, 3, 2, 1};              // the max-pool's window
    for (int i = 0; i < kUnetNodes; ++i) {
        const UnetNode &n = nodes[i];
        const UnetConvDesc &d = n.out == kUnetPool ? pool : layers[n.out];
        const int up = n.upsample ? 2 : 1, hin = (n.in == kUnetColors ? H : g[n.in].hout) * up, win = (n.in == kUnetColors ? W : g[n.in].wout) * up;
        g[n.out] = {hin, win, (hin + 2 * d.pad - d.ksize) / d.stride + 1, (win + 2 * d.pad - d.ksize) / d.stride + 1};
    }
    return g;
}

}  // namespace bn
