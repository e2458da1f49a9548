// unet_host.cpp -- the C ABI of the U-Net terrain classifier (include/benchnav_mppi.h): argument checks, the
// parameter upload and re-layout, the workspace plan and the launch sequence of one forward.  Kernels: unet_kernels.hip.
#include <cmath>
#include <cstring>
#include <string>

#include "unet_handle.h"

namespace bn {
namespace {

thread_local std::string g_unet_error;

int unet_fail(int code, const std::string &msg)
{
    g_unet_error = msg;
    return code;
}

#define UNET_HIP(expr) BN_HIP_AS(unet_fail, expr, #expr)

size_t unet_align(size_t v) { return (v + 255) & ~(size_t)255; }

bool unet_shape_ok(int64_t num_maps, int64_t H, int64_t W)
{
    return num_maps >= 1 && num_maps <= kUnetMaxMaps && H >= kUnetMinSide && H <= kUnetMaxSide && W >= kUnetMinSide && W <= kUnetMaxSide &&
           H % 32 == 0 && W % 32 == 0 && num_maps * H * W <= kUnetMaxPixels;
}

// Where every activation of one forward lives in the workspace (byte offsets, each a multiple of 256).
struct UnetPlan {
    size_t stem = 0, pool = 0, lt[4] = {}, ld[4] = {}, lb[4] = {}, lo[4] = {}, dt[5] = {}, dout[5] = {}, logits = 0, total = 0;
};

constexpr int kWidth[4] = {64, 128, 256, 512};
constexpr int kDecIn[5] = {512, 256, 128, 64, 32}, kDecSkip[5] = {256, 128, 64, 64, 0}, kDecOut[5] = {256, 128, 64, 32, 16};

UnetPlan unet_plan(int64_t n, int64_t H, int64_t W)
{
    UnetPlan p;
    size_t at = 0;
    auto take = [&](int64_t channels, int64_t h, int64_t w) {
        const size_t o = at;
        at += unet_align((size_t)(n * channels * h * w) * sizeof(float));
        return o;
    };
    p.stem = take(64, H / 2, W / 2);
    p.pool = take(64, H / 4, W / 4);
    for (int l = 0; l < 4; ++l) {
        const int64_t h = H >> (2 + l), w = W >> (2 + l);
        p.lt[l] = take(kWidth[l], h, w);
        if (l) p.ld[l] = take(kWidth[l], h, w);
        p.lb[l] = take(kWidth[l], h, w);
        p.lo[l] = take(kWidth[l], h, w);
    }
    for (int b = 0; b < 5; ++b) {
        const int64_t h = H >> (4 - b), w = W >> (4 - b);
        p.dt[b] = take(kDecOut[b], h, w);
        p.dout[b] = take(kDecOut[b], h, w);
    }
    p.logits = take(kUnetMaxClasses, H, W);
    p.total = at;
    return p;
}

int unet_open_device(int32_t device_id)
{
    return open_device(device_id, unet_fail);
}

}  // namespace
}  // namespace bn

using bn::unet_fail;

extern "C" {

const char *bn_unet_last_error(void) { return bn::g_unet_error.c_str(); }

int64_t bn_unet_param_count(int32_t classes)
{
    if (classes < 1 || classes > bn::kUnetMaxClasses) return 0;
    int64_t n = 0;
    for (const bn::UnetConvDesc &d : bn::unet_layers(classes)) n += (int64_t)d.host_floats();
    return n;
}

int bn_unet_create(int32_t device_id, int32_t classes, const float *params_host, int64_t count, bn_unet_t **out)
{
    if (!out) return unet_fail(BN_ERR_INVALID, "null handle pointer");
    *out = nullptr;
    if (classes < 1 || classes > bn::kUnetMaxClasses) return unet_fail(BN_ERR_INVALID, "classes must be in [1, " + std::to_string(bn::kUnetMaxClasses) + "]");
    if (!params_host) return unet_fail(BN_ERR_INVALID, "null argument");
    if (count != bn_unet_param_count(classes))
        return unet_fail(BN_ERR_INVALID, "count must be bn_unet_param_count(classes) = " + std::to_string(bn_unet_param_count(classes)));
    for (int64_t i = 0; i < count; ++i)
        if (!std::isfinite(params_host[i])) return unet_fail(BN_ERR_INVALID, "every parameter must be finite (index " + std::to_string(i) + ")");
    if (int rc = bn::unet_open_device(device_id)) return rc;
    BN_ON_DEVICE(unet_fail, device_id);

    bn_unet *h = new bn_unet();
    h->device = device_id;
    h->classes = classes;
    h->layers = bn::unet_layers(classes);
    size_t total = 0;
    for (const bn::UnetConvDesc &d : h->layers) {
        h->offset.push_back(total);
        total += d.device_floats();
    }
    float *raw = nullptr;
    h->bufs.add(&h->weights, total * sizeof(float));
    h->bufs.add(&raw, (size_t)count * sizeof(float));
    auto run = [&]() -> int {
        if (int rc = h->bufs.alloc_all(unet_fail)) return rc;
        UNET_HIP(hipMemcpy(raw, params_host, (size_t)count * sizeof(float), hipMemcpyHostToDevice));
        size_t at = 0;
        for (size_t i = 0; i < h->layers.size(); ++i) {
            const bn::UnetConvDesc &d = h->layers[i];
            float *wt = h->weights + h->offset[i];
            UNET_HIP(bn::unet_launch_relayout(nullptr, raw + at, raw + at + (size_t)d.cout * d.K(), wt, wt + (size_t)d.kpad() * d.coutpad(), d.cout,
                                              d.K(), d.kpad(), d.coutpad()));
            at += d.host_floats();
        }
        UNET_HIP(hipStreamSynchronize(nullptr));
        return BN_OK;
    };
    int rc = run();
    if (rc != BN_OK) {
        h->bufs.free_all();
        delete h;
        return rc;
    }
    (void)hipFree(raw);
    h->bufs.list.pop_back();                             // the staging copy is gone; the handle keeps the re-laid weights only
    *out = h;
    return BN_OK;
}

void bn_unet_destroy(bn_unet_t *h)
{
    if (!h) return;
    {
        bn::DeviceGuard guard(h->device);
        h->bufs.free_all();
    }
    delete h;
}

size_t bn_unet_workspace_bytes(int32_t num_maps, int32_t H, int32_t W)
{
    if (!bn::unet_shape_ok(num_maps, H, W)) return 0;
    return bn::unet_plan(num_maps, H, W).total;
}

int bn_unet_feature_layout(int32_t num_maps, int32_t H, int32_t W, int32_t index, size_t *offset_bytes, int32_t *channels, int32_t *height,
                           int32_t *width)
{
    if (!offset_bytes || !channels || !height || !width) return unet_fail(BN_ERR_INVALID, "null argument");
    if (!bn::unet_shape_ok(num_maps, H, W)) return unet_fail(BN_ERR_INVALID, "num_maps, H or W out of range (H and W must be multiples of 32)");
    if (index < 0 || index > 9) return unet_fail(BN_ERR_INVALID, "feature index must be in [0, 9]");
    const bn::UnetPlan p = bn::unet_plan(num_maps, H, W);
    if (index == 0) { *offset_bytes = p.stem; *channels = 64; *height = H / 2; *width = W / 2; }
    else if (index <= 4) { const int l = index - 1; *offset_bytes = p.lo[l]; *channels = bn::kWidth[l]; *height = H >> (2 + l); *width = W >> (2 + l); }
    else { const int b = index - 5; *offset_bytes = p.dout[b]; *channels = bn::kDecOut[b]; *height = H >> (4 - b); *width = W >> (4 - b); }
    return BN_OK;
}

int bn_unet_forward_async(bn_unet_t *h, void *stream, int32_t num_maps, int32_t H, int32_t W, const float *colors_device, float *logits_device,
                          float *probabilities_device, int32_t *classes_device, void *workspace_device, size_t workspace_bytes)
{
    if (!h || !colors_device || !workspace_device) return unet_fail(BN_ERR_INVALID, "null argument");
    if (!bn::unet_shape_ok(num_maps, H, W))
        return unet_fail(BN_ERR_INVALID, "H and W must be multiples of 32 in [32, 2048], num_maps in [1, 4096], num_maps H W <= 2^24");
    const bn::UnetPlan p = bn::unet_plan(num_maps, H, W);
    if (workspace_bytes < p.total) return unet_fail(BN_ERR_INVALID, "workspace smaller than bn_unet_workspace_bytes(num_maps, H, W)");
    BN_ON_DEVICE(unet_fail, h->device);
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace_device;
    auto buf = [&](size_t off) { return (float *)(ws + off); };

    // one fused convolution of the table: input a (ca channels, optionally upsampled) ++ b (cb channels) of hin x win
    auto conv = [&](int layer, const float *a, int ca, const float *b, int cb, int upsample, int hin, int win, const float *residual, int relu,
                    float *out) -> hipError_t {
        const bn::UnetConvDesc &d = h->layers[layer];
        bn::UnetConvArgs g{};
        g.a = a; g.b = b;
        g.wt = h->weights + h->offset[layer];
        g.bias = g.wt + (size_t)d.kpad() * d.coutpad();
        g.residual = residual; g.out = out;
        g.num_maps = num_maps; g.ca = ca; g.cb = cb; g.hin = hin; g.win = win;
        g.hout = (hin + 2 * d.pad - d.ksize) / d.stride + 1;
        g.wout = (win + 2 * d.pad - d.ksize) / d.stride + 1;
        g.cout = d.cout; g.coutpad = d.coutpad(); g.k = d.K(); g.kpad = d.kpad(); g.stride = d.stride; g.pad = d.pad;
        g.upsample = upsample; g.relu = relu;
        return bn::unet_launch_conv(s, d.ksize, g);
    };

    UNET_HIP(conv(bn::kUnetStem, colors_device, 3, nullptr, 0, 0, H, W, nullptr, 1, buf(p.stem)));
    UNET_HIP(bn::unet_launch_maxpool(s, buf(p.stem), buf(p.pool), (int64_t)num_maps * 64, H / 2, W / 2, H / 4, W / 4));
    const int first[4] = {bn::kUnetLayer1, bn::kUnetLayer2, bn::kUnetLayer3, bn::kUnetLayer4};
    const float *x = buf(p.pool);
    int cin = 64, hin = H / 4, win = W / 4;
    for (int l = 0; l < 4; ++l) {
        const int w = bn::kWidth[l], i = first[l], ho = l ? hin / 2 : hin, wo = l ? win / 2 : win;
        const float *identity = x;
        UNET_HIP(conv(i, x, cin, nullptr, 0, 0, hin, win, nullptr, 1, buf(p.lt[l])));
        if (l) {
            UNET_HIP(conv(i + 2, x, cin, nullptr, 0, 0, hin, win, nullptr, 0, buf(p.ld[l])));
            identity = buf(p.ld[l]);
        }
        UNET_HIP(conv(i + 1, buf(p.lt[l]), w, nullptr, 0, 0, ho, wo, identity, 1, buf(p.lb[l])));
        const int j = l ? i + 3 : i + 2;
        UNET_HIP(conv(j, buf(p.lb[l]), w, nullptr, 0, 0, ho, wo, nullptr, 1, buf(p.lt[l])));
        UNET_HIP(conv(j + 1, buf(p.lt[l]), w, nullptr, 0, 0, ho, wo, buf(p.lb[l]), 1, buf(p.lo[l])));
        x = buf(p.lo[l]);
        cin = w; hin = ho; win = wo;
    }
    const size_t skip[5] = {p.lo[2], p.lo[1], p.lo[0], p.stem, 0};
    for (int b = 0; b < 5; ++b) {
        const int ho = hin * 2, wo = win * 2, i = bn::kUnetDecoder + 2 * b;
        UNET_HIP(conv(i, x, bn::kDecIn[b], bn::kDecSkip[b] ? buf(skip[b]) : nullptr, bn::kDecSkip[b], 1, ho, wo, nullptr, 1, buf(p.dt[b])));
        UNET_HIP(conv(i + 1, buf(p.dt[b]), bn::kDecOut[b], nullptr, 0, 0, ho, wo, nullptr, 1, buf(p.dout[b])));
        x = buf(p.dout[b]);
        hin = ho; win = wo;
    }
    float *logits = logits_device ? logits_device : buf(p.logits);
    UNET_HIP(conv(bn::kUnetHead, x, 16, nullptr, 0, 0, H, W, nullptr, 0, logits));
    if (probabilities_device || classes_device)
        UNET_HIP(bn::unet_launch_head(s, logits, probabilities_device, classes_device, num_maps, h->classes, (int64_t)H * W));
    return BN_OK;
}

size_t bn_unet_conv2d_workspace_bytes(int32_t cin, int32_t cout, int32_t ksize)
{
    if (cin < 1 || cin > 4096 || cout < 1 || cout > 4096 || (ksize != 1 && ksize != 3 && ksize != 7)) return 0;
    const bn::UnetConvDesc d{cin, cout, ksize, 1, 0};
    return bn::unet_align(d.device_floats() * sizeof(float));
}

int bn_unet_conv2d_async(int32_t device_id, void *stream, const float *a_device, int32_t ca, const float *skip_device, int32_t cb, int32_t upsample,
                         int32_t num_maps, int32_t hin, int32_t win, const float *weights_device, const float *bias_device, int32_t cout,
                         int32_t ksize, int32_t stride, int32_t pad, const float *residual_device, int32_t relu, float *out_device,
                         void *workspace_device, size_t workspace_bytes)
{
    if (!a_device || !weights_device || !out_device || !workspace_device) return unet_fail(BN_ERR_INVALID, "null argument");
    if (ca < 1 || cb < 0 || (cb > 0 && !skip_device)) return unet_fail(BN_ERR_INVALID, "ca must be >= 1, cb >= 0, and cb > 0 needs the skip tensor");
    if (ksize != 1 && ksize != 3 && ksize != 7) return unet_fail(BN_ERR_INVALID, "ksize must be 1, 3 or 7");
    if (stride < 1 || stride > 2 || pad < 0 || pad > 3) return unet_fail(BN_ERR_INVALID, "stride must be 1 or 2 and pad in [0, 3]");
    const size_t need = bn_unet_conv2d_workspace_bytes(ca + cb, cout, ksize);
    if (need == 0) return unet_fail(BN_ERR_INVALID, "input and output channels must be in [1, 4096]");
    if (workspace_bytes < need) return unet_fail(BN_ERR_INVALID, "workspace smaller than bn_unet_conv2d_workspace_bytes(cin, cout, ksize)");
    if (num_maps < 1 || num_maps > bn::kUnetMaxMaps || hin < 1 || hin > bn::kUnetMaxSide || win < 1 || win > bn::kUnetMaxSide)
        return unet_fail(BN_ERR_INVALID, "num_maps must be in [1, 4096] and the input sides in [1, 2048]");
    if (upsample != 0 && upsample != 1) return unet_fail(BN_ERR_INVALID, "upsample must be 0 or 1");
    if (upsample && ((hin | win) & 1)) return unet_fail(BN_ERR_INVALID, "an upsampled input has even sides");
    const int hout = (hin + 2 * pad - ksize) / stride + 1, wout = (win + 2 * pad - ksize) / stride + 1;
    if (hin + 2 * pad < ksize || win + 2 * pad < ksize) return unet_fail(BN_ERR_INVALID, "the kernel does not fit the padded input");
    if ((int64_t)num_maps * hin * win > bn::kUnetMaxPixels || (int64_t)num_maps * hout * wout > bn::kUnetMaxPixels)
        return unet_fail(BN_ERR_INVALID, "num_maps x pixels must be <= 2^24");
    if ((int64_t)num_maps * (ca + cb) * hin * win >= ((int64_t)1 << 31) || (int64_t)num_maps * cout * hout * wout >= ((int64_t)1 << 31))
        return unet_fail(BN_ERR_INVALID, "a tensor must hold fewer than 2^31 elements");
    if (int rc = bn::unet_open_device(device_id)) return rc;
    BN_ON_DEVICE(unet_fail, device_id);
    hipStream_t s = (hipStream_t)stream;
    const bn::UnetConvDesc d{ca + cb, cout, ksize, stride, pad};
    float *wt = (float *)workspace_device, *bias = wt + (size_t)d.kpad() * d.coutpad();
    UNET_HIP(bn::unet_launch_relayout(s, weights_device, bias_device, wt, bias, cout, d.K(), d.kpad(), d.coutpad()));
    bn::UnetConvArgs g{};
    g.a = a_device; g.b = skip_device; g.wt = wt; g.bias = bias; g.residual = residual_device; g.out = out_device;
    g.num_maps = num_maps; g.ca = ca; g.cb = cb; g.hin = hin; g.win = win; g.hout = hout; g.wout = wout;
    g.cout = cout; g.coutpad = d.coutpad(); g.k = d.K(); g.kpad = d.kpad(); g.stride = stride; g.pad = pad;
    g.upsample = upsample; g.relu = relu ? 1 : 0;
    UNET_HIP(bn::unet_launch_conv(s, ksize, g));
    return BN_OK;
}

int bn_unet_maxpool_async(int32_t device_id, void *stream, const float *in_device, int64_t planes, int32_t hin, int32_t win, float *out_device)
{
    if (!in_device || !out_device) return unet_fail(BN_ERR_INVALID, "null argument");
    if (planes < 1 || hin < 1 || hin > bn::kUnetMaxSide || win < 1 || win > bn::kUnetMaxSide || planes * hin * win > ((int64_t)1 << 30))
        return unet_fail(BN_ERR_INVALID, "planes must be >= 1, the sides in [1, 2048] and planes x hin x win <= 2^30");
    if (int rc = bn::unet_open_device(device_id)) return rc;
    BN_ON_DEVICE(unet_fail, device_id);
    UNET_HIP(bn::unet_launch_maxpool((hipStream_t)stream, in_device, out_device, planes, hin, win, (hin - 1) / 2 + 1, (win - 1) / 2 + 1));
    return BN_OK;
}

}  // extern "C"
