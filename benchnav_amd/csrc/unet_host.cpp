// unet_host.cpp -- the C ABI of the U-Net terrain classifier (include/benchnav_mppi.h): argument checks, the
// parameter upload and re-layout, the workspace plan and one forward: a walk over the nodes of unet_graph.h.  Kernels:
// unet_kernels.hip.
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

bool unet_shape_ok(int64_t num_maps, int64_t H, int64_t W)
{
    return num_maps >= 1 && num_maps <= kUnetMaxMaps && H >= kUnetMinSide && H <= kUnetMaxSide && W >= kUnetMinSide && W <= kUnetMaxSide &&
           H % 32 == 0 && W % 32 == 0 && num_maps * H * W <= kUnetMaxPixels;
}

// Where every activation of one forward lives in the workspace (byte offsets by slot, each a multiple of 256): one block per node
// in execution order, except where a node reuses another's; the head's block holds logits of kUnetMaxClasses channels.
struct UnetPlan {
    size_t at[kUnetSlots] = {}, total = 0;
};

UnetPlan unet_plan(const std::vector<UnetConvDesc> &layers, const std::vector<UnetGeo> &geo, int64_t n)
{
    UnetPlan p;
    const UnetNode *nodes = unet_nodes();
    for (int i = 0; i < kUnetNodes; ++i) {
        const UnetNode &nd = nodes[i];
        if (nd.reuse != kUnetNone) {
            p.at[nd.out] = p.at[nd.reuse];
            continue;
        }
        const int64_t channels = nd.out == kUnetHead ? kUnetMaxClasses : unet_channels(layers, nd.out);
        p.at[nd.out] = p.total;
        p.total += unet_align((size_t)(n * channels * geo[nd.out].hout * geo[nd.out].wout) * sizeof(float));
    }
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
    const std::vector<bn::UnetConvDesc> layers = bn::unet_layers(bn::kUnetMaxClasses);
    return bn::unet_plan(layers, bn::unet_geometry(layers, H, W), num_maps).total;
}

int bn_unet_feature_layout(int32_t num_maps, int32_t H, int32_t W, int32_t index, size_t *offset_bytes, int32_t *channels, int32_t *height,
                           int32_t *width)
{
    if (!offset_bytes || !channels || !height || !width) return unet_fail(BN_ERR_INVALID, "null argument");
    if (!bn::unet_shape_ok(num_maps, H, W)) return unet_fail(BN_ERR_INVALID, "num_maps, H or W out of range (H and W must be multiples of 32)");
    if (index < 0 || index > 9) return unet_fail(BN_ERR_INVALID, "feature index must be in [0, 9]");
    const std::vector<bn::UnetConvDesc> layers = bn::unet_layers(bn::kUnetMaxClasses);
    const std::vector<bn::UnetGeo> geo = bn::unet_geometry(layers, H, W);
    const int slot = bn::kUnetFeatures[index];
    *offset_bytes = bn::unet_plan(layers, geo, num_maps).at[slot];
    *channels = layers[slot].cout;
    *height = geo[slot].hout;
    *width = geo[slot].wout;
    return BN_OK;
}

int bn_unet_forward_async(bn_unet_t *h, void *stream, int32_t num_maps, int32_t H, int32_t W, const float *colors_device, float *logits_device,
                          float *probabilities_device, int32_t *classes_device, void *workspace_device, size_t workspace_bytes)
{
    if (!h || !colors_device || !workspace_device) return unet_fail(BN_ERR_INVALID, "null argument");
    if (!bn::unet_shape_ok(num_maps, H, W))
        return unet_fail(BN_ERR_INVALID, "H and W must be multiples of 32 in [32, 2048], num_maps in [1, 4096], num_maps H W <= 2^24");
    const std::vector<bn::UnetConvDesc> any = bn::unet_layers(bn::kUnetMaxClasses);     // sizes are checked before the handle is read
    const std::vector<bn::UnetGeo> geo = bn::unet_geometry(any, H, W);
    const bn::UnetPlan p = bn::unet_plan(any, geo, num_maps);
    if (workspace_bytes < p.total) return unet_fail(BN_ERR_INVALID, "workspace smaller than bn_unet_workspace_bytes(num_maps, H, W)");
    BN_ON_DEVICE(unet_fail, h->device);
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace_device;
    float *logits = logits_device ? logits_device : (float *)(ws + p.at[bn::kUnetHead]);
    auto buf = [&](int slot) { return slot == bn::kUnetHead ? logits : (float *)(ws + p.at[slot]); };
    auto src = [&](int slot) -> const float * { return slot == bn::kUnetNone ? nullptr : slot == bn::kUnetColors ? colors_device : buf(slot); };

    const bn::UnetNode *nodes = bn::unet_nodes();
    for (int i = 0; i < bn::kUnetNodes; ++i) {
        const bn::UnetNode &n = nodes[i];
        const bn::UnetGeo &g = geo[n.out];
        const int ca = bn::unet_channels(h->layers, n.in);
        if (n.out == bn::kUnetPool) {
            UNET_HIP(bn::unet_launch_maxpool(s, src(n.in), buf(n.out), (int64_t)num_maps * ca, g.hin, g.win, g.hout, g.wout));
            continue;
        }
        const bn::UnetConvDesc &d = h->layers[n.out];
        UNET_HIP(bn::unet_launch_conv(s, d.ksize, bn::unet_conv_args(d, g, num_maps, src(n.in), ca, src(n.skip), n.upsample, h->weights + h->offset[n.out],
                                                                     src(n.residual), n.relu, buf(n.out))));
    }
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
    if (cb > 0 && !skip_device) return unet_fail(BN_ERR_INVALID, "cb > 0 needs the skip tensor");
    if (const char *why = bn::unet_conv_check(ca, cb, cout, ksize, stride, pad, upsample, num_maps, hin, win, false)) return unet_fail(BN_ERR_INVALID, why);
    if (workspace_bytes < bn_unet_conv2d_workspace_bytes(ca + cb, cout, ksize))
        return unet_fail(BN_ERR_INVALID, "workspace smaller than bn_unet_conv2d_workspace_bytes(cin, cout, ksize)");
    if (int rc = bn::unet_open_device(device_id)) return rc;
    BN_ON_DEVICE(unet_fail, device_id);
    hipStream_t s = (hipStream_t)stream;
    const bn::UnetConvDesc d{ca + cb, cout, ksize, stride, pad};
    const bn::UnetGeo geo{hin, win, (hin + 2 * pad - ksize) / stride + 1, (win + 2 * pad - ksize) / stride + 1};
    float *wt = (float *)workspace_device;
    UNET_HIP(bn::unet_launch_relayout(s, weights_device, bias_device, wt, wt + (size_t)d.kpad() * d.coutpad(), cout, d.K(), d.kpad(), d.coutpad()));
    UNET_HIP(bn::unet_launch_conv(s, ksize, bn::unet_conv_args(d, geo, num_maps, a_device, ca, skip_device, upsample, wt, residual_device, relu ? 1 : 0,
                                                               out_device)));
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
