// segtrain_host.cpp -- the C ABI that trains the U-Net terrain classifier (include/benchnav_mppi.h): argument
// checks, the parameter layout, the workspace plan, one training-mode forward + loss + backward as two walks over the nodes of
// unet_graph.h, Adam, and the single-layer entry points the layer tests drive.  Kernels: segtrain_kernels.hip and
// unet_kernels.hip's convolution.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "segtrain_handle.h"

namespace bn {
namespace {

thread_local std::string g_seg_error;

int seg_fail(int code, const std::string &msg)
{
    g_seg_error = msg;
    return code;
}

#define SEG_HIP(expr) BN_HIP_AS(seg_fail, expr, #expr)

// bn_unet_workspace_bytes' range, and more than one value per channel at the bottleneck (BatchNorm in training mode)
bool seg_shape_ok(int64_t num_maps, int64_t H, int64_t W)
{
    return num_maps >= 1 && num_maps <= kUnetMaxMaps && H >= kUnetMinSide && H <= kUnetMaxSide && W >= kUnetMinSide && W <= kUnetMaxSide &&
           H % 32 == 0 && W % 32 == 0 && num_maps * H * W <= kUnetMaxPixels && num_maps * (H / 32) * (W / 32) > 1;
}

size_t seg_flip_floats(int cin, int cout, int ksize)
{
    const size_t cinpad = unet_round_up(cin, kUnetTile);
    return (size_t)unet_round_up(cout * ksize * ksize, kUnetKStep) * cinpad + cinpad;
}

size_t seg_partial_floats(int64_t npix, int cout, int k) { return (size_t)seg_split(npix, cout, k).chunks * cout * k; }

// Where everything one step keeps lives in the workspace (byte offsets by slot of unet_graph.h, multiples of 256): per convolution
// its raw output c, the activation y behind BatchNorm and the gradient g (of y, then in place of c), and the batch statistics as
// float64.  The head's c are the logits and its g their gradient; the pool has a y and a g.
struct SegPlan {
    size_t c[kUnetSlots] = {}, y[kUnetSlots] = {}, g[kUnetSlots] = {}, stats[kUnetConvs] = {};
    size_t dcat = 0, flip = 0, partial = 0, sums = 0, terms = 0, total = 0;
};

SegPlan seg_plan(const std::vector<UnetConvDesc> &layers, const std::vector<UnetGeo> &geo, int64_t n, int H, int W)
{
    SegPlan p;
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t o = at;
        at += unet_align(bytes);
        return o;
    };
    size_t flip = 0, partial = 0, dcat = 0, widest = 0;
    for (int i = 0; i < kUnetConvs; ++i) {
        const UnetConvDesc &d = layers[i];
        const size_t act = (size_t)(n * d.cout * geo[i].hout * geo[i].wout) * sizeof(float);
        if (i < kUnetHead) {
            p.c[i] = take(act);
            p.y[i] = take(act);
            p.g[i] = take(act);
            p.stats[i] = take((size_t)2 * d.cout * sizeof(double));
            widest = std::max(widest, (size_t)d.cout);
        }
        if (i) flip = std::max(flip, seg_flip_floats(d.cin, d.cout, d.ksize));
        partial = std::max(partial, seg_partial_floats(n * geo[i].hout * geo[i].wout, d.cout, d.K()));
    }
    const size_t pool = (size_t)(n * unet_channels(layers, kUnetPool) * geo[kUnetPool].hout * geo[kUnetPool].wout) * sizeof(float);
    p.y[kUnetPool] = take(pool);
    p.g[kUnetPool] = take(pool);
    p.c[kUnetHead] = take((size_t)(n * kUnetMaxClasses * H * W) * sizeof(float));
    p.g[kUnetHead] = take((size_t)(n * kUnetMaxClasses * H * W) * sizeof(float));
    const UnetNode *nodes = unet_nodes();
    for (int i = 0; i < kUnetNodes; ++i)                 // the data gradient of a concatenated or upsampled input is split from here
        if (nodes[i].skip != kUnetNone || nodes[i].upsample)
            dcat = std::max(dcat, (size_t)(n * layers[nodes[i].out].cin * geo[nodes[i].out].hin * geo[nodes[i].out].win));
    p.dcat = take(dcat * sizeof(float));
    p.flip = take(flip * sizeof(float));
    p.partial = take(partial * sizeof(float));
    p.sums = take(2 * widest * sizeof(double));
    p.terms = take((size_t)(n * H * W) * sizeof(double));
    p.total = at;
    return p;
}

int seg_open_device(int32_t device_id) { return open_device(device_id, seg_fail); }

// The host's parameter order: per convolution its weight, gamma and beta (the head: its bias) -- `train` floats at `at` -- and behind
// them the running mean and variance, `stats` floats (the head: none).
struct SegHostSpan { size_t at, train, stats; };

std::vector<SegHostSpan> seg_host_order(const std::vector<UnetConvDesc> &layers, int64_t *total)
{
    std::vector<SegHostSpan> v;
    size_t at = 0;
    for (int i = 0; i < kUnetConvs; ++i) {
        const size_t cout = layers[i].cout, bn = i == kUnetHead ? 0 : 2 * cout;
        v.push_back({at, cout * layers[i].K() + (bn ? bn : cout), bn});
        at += v.back().train + bn;
    }
    *total = (int64_t)at;
    return v;
}

bool seg_adam_ok(double lr, double beta1, double beta2, double eps, double weight_decay)
{
    if (lr >= 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0 && weight_decay >= 0.0 && std::isfinite(lr) &&
        std::isfinite(eps) && std::isfinite(weight_decay))
        return true;
    seg_fail(BN_ERR_INVALID, "lr, eps and weight_decay must be finite and >= 0, beta1 and beta2 in [0, 1)");
    return false;
}

bool seg_bn_shape_ok(int64_t num_maps, int64_t channels, int64_t cells)
{
    if (num_maps >= 1 && channels >= 1 && channels <= 4096 && cells >= 1 && num_maps * cells <= kUnetMaxPixels && num_maps * cells >= 2 &&
        num_maps * cells * channels < ((int64_t)1 << 31))
        return true;
    seg_fail(BN_ERR_INVALID, "channels must be in [1, 4096], num_maps x cells in [2, 2^24] (more than 1 value per channel), the tensor < 2^31");
    return false;
}

// dX = backward-data of convolution d into `out` (num_maps, cin, hin, win), plus `residual` where given: stride 1 through the
// forward convolution on the flipped weight, stride 2 through the strided kernel.  `flip` is scratch for that weight.
hipError_t seg_dgrad(hipStream_t s, const UnetConvDesc &d, const UnetGeo &geo, int num_maps, const float *w, const float *dy, const float *residual,
                     float *out, float *flip)
{
    const UnetConvDesc t{d.cout, d.cin, d.ksize, 1, d.ksize - 1 - d.pad};      // the transposed convolution: dy in, dx out
    if (hipError_t e = seg_launch_flip(s, w, flip, flip + (size_t)t.kpad() * t.coutpad(), d.cout, d.cin, d.ksize, t.kpad(), t.coutpad())) return e;
    if (d.stride == 1)
        return unet_launch_conv(s, d.ksize, unet_conv_args(t, UnetGeo{geo.hout, geo.wout, geo.hin, geo.win}, num_maps, dy, d.cout, nullptr, 0, flip,
                                                           residual, 0, out));
    SegConvGrad g{};
    g.dy = dy; g.wt = flip; g.residual = residual; g.out = out;
    g.num_maps = num_maps; g.ca = d.cin; g.cb = 0; g.hin = geo.hin; g.win = geo.win; g.hout = geo.hout; g.wout = geo.wout;
    g.cout = d.cout; g.k = t.K(); g.kpad = t.kpad(); g.cinpad = t.coutpad(); g.stride = d.stride; g.pad = d.pad;
    return seg_launch_dgrad_strided(s, d.ksize, g);
}

// dW = backward-weight of convolution d on the input a (ca channels, optionally upsampled) ++ b: the partial sums into `partial`,
// then their sum in ascending chunk order into dw
hipError_t seg_wgrad(hipStream_t s, const UnetConvDesc &d, const UnetGeo &geo, int num_maps, const float *a, int ca, const float *b, int upsample,
                     const float *dy, float *partial, float *dw)
{
    SegConvGrad g{};
    g.a = a; g.b = b; g.dy = dy; g.out = partial;
    g.num_maps = num_maps; g.ca = ca; g.cb = d.cin - ca; g.hin = geo.hin; g.win = geo.win; g.hout = geo.hout; g.wout = geo.wout;
    g.cout = d.cout; g.k = d.K(); g.stride = d.stride; g.pad = d.pad; g.upsample = upsample;
    const SegSplit sp = seg_split((int64_t)num_maps * geo.hout * geo.wout, d.cout, g.k);
    g.chunks = sp.chunks; g.stages = sp.stages;
    if (hipError_t e = seg_launch_wgrad(s, d.ksize, g)) return e;
    return seg_launch_wgrad_reduce(s, partial, dw, (int64_t)d.cout * g.k, sp.chunks);
}

// One training-mode forward, the loss and the backward on `s`; the gradients end in h->grads.  Both are walks over the nodes of
// unet_graph.h: forwards, then in reverse.
int seg_run(bn_segtrain *h, hipStream_t s, int B, int H, int W, const float *colors, const int64_t *targets, float *loss, char *ws, bool update_stats)
{
    const std::vector<UnetGeo> geo = unet_geometry(h->layers, H, W);
    const SegPlan p = seg_plan(h->layers, geo, B, H, W);
    const UnetNode *nodes = unet_nodes();
    auto C = [&](int i) { return (float *)(ws + p.c[i]); };
    auto G = [&](int i) { return (float *)(ws + p.g[i]); };
    auto Y = [&](int i) -> const float * { return i == kUnetNone ? nullptr : i == kUnetColors ? colors : (const float *)(ws + p.y[i]); };
    float *dcat = (float *)(ws + p.dcat), *flip = (float *)(ws + p.flip), *partial = (float *)(ws + p.partial);
    double *sums = (double *)(ws + p.sums), *terms = (double *)(ws + p.terms);
    auto stats = [&](int i) { return (double *)(ws + p.stats[i]); };
    auto cells = [&](int i) { return (int64_t)geo[i].hout * geo[i].wout; };
    auto weight = [&](int i) { return h->params + h->weight_at[i]; };
    auto gamma = [&](int i) { return weight(i) + (size_t)h->layers[i].cout * h->layers[i].K(); };
    auto wgrad_at = [&](int i) { return h->grads + h->weight_at[i]; };

    // the forward reads the weights as unet_conv_kernel does: re-laid from the current parameters, a zero bias except the head's
    for (int i = 0; i < kUnetConvs; ++i) {
        const UnetConvDesc &d = h->layers[i];
        float *wt = h->wt + h->wt_at[i];
        SEG_HIP(unet_launch_relayout(s, weight(i), i == kUnetHead ? gamma(i) : nullptr, wt, wt + (size_t)d.kpad() * d.coutpad(), d.cout, d.K(), d.kpad(),
                                     d.coutpad()));
    }
    for (int k = 0; k < kUnetNodes; ++k) {
        const UnetNode &n = nodes[k];
        const int i = n.out, ca = unet_channels(h->layers, n.in);
        if (i == kUnetPool) {
            SEG_HIP(unet_launch_maxpool(s, Y(n.in), (float *)(ws + p.y[i]), (int64_t)B * ca, geo[i].hin, geo[i].win, geo[i].hout, geo[i].wout));
            continue;
        }
        const UnetConvDesc &d = h->layers[i];
        SEG_HIP(unet_launch_conv(s, d.ksize, unet_conv_args(d, geo[i], B, Y(n.in), ca, Y(n.skip), n.upsample, h->wt + h->wt_at[i], nullptr, 0, C(i))));
        if (i == kUnetHead) continue;                    // the head has a bias and no BatchNorm: C(head) are the logits
        float *rm = update_stats ? h->params + h->stats_at[i] : nullptr;
        SEG_HIP(seg_launch_bn_forward(s, C(i), gamma(i), gamma(i) + d.cout, Y(n.residual), n.relu, rm, rm ? rm + d.cout : nullptr, (float *)(ws + p.y[i]),
                                      stats(i), B, d.cout, cells(i)));
    }
    SEG_HIP(seg_launch_cross_entropy(s, C(kUnetHead), targets, G(kUnetHead), terms, loss, B, h->classes, (int64_t)H * W));

    // ---- backward: per node BatchNorm's backward in place (the residual's gradient goes to its source's G), the weight gradient,
    // and the data gradient into the input's G.  A gradient buffer's first writer stores, the later ones add. ----
    bool written[kUnetSlots] = {};
    auto add_into = [&](int slot) {
        const bool add = written[slot];
        written[slot] = true;
        return add;
    };
    for (int k = kUnetNodes - 1; k >= 0; --k) {
        const UnetNode &n = nodes[k];
        const int i = n.out, ca = unet_channels(h->layers, n.in);
        if (i == kUnetPool) {
            SEG_HIP(seg_launch_maxpool_backward(s, Y(n.in), G(i), G(n.in), (int64_t)B * ca, geo[i].hin, geo[i].win, add_into(n.in)));
            continue;
        }
        const UnetConvDesc &d = h->layers[i];
        float *bn_grads = wgrad_at(i) + (size_t)d.cout * d.K();           // gamma's and beta's gradient; the head: its bias's
        if (i != kUnetHead) {
            // BatchNorm's backward only stores the residual's gradient: it must be that buffer's first writer
            if (n.residual != kUnetNone && add_into(n.residual)) return seg_fail(BN_ERR_INVALID, "the graph adds a residual gradient to a written buffer");
            SEG_HIP(seg_launch_bn_backward(s, G(i), Y(i), C(i), stats(i), gamma(i), n.relu, G(i), n.residual != kUnetNone ? G(n.residual) : nullptr, bn_grads,
                                           bn_grads + d.cout, sums, B, d.cout, cells(i)));
        }
        SEG_HIP(seg_wgrad(s, d, geo[i], B, Y(n.in), ca, Y(n.skip), n.upsample, G(i), partial, wgrad_at(i)));
        if (i == kUnetHead) SEG_HIP(seg_launch_bias_grad(s, G(i), bn_grads, B, d.cout, cells(i)));
        if (n.in == kUnetColors) continue;
        if (n.skip == kUnetNone && !n.upsample) {
            float *out = G(n.in);
            SEG_HIP(seg_dgrad(s, d, geo[i], B, weight(i), G(i), add_into(n.in) ? out : nullptr, out, flip));
            continue;
        }
        // the split writes both halves one way
        const bool add = add_into(n.in);
        if (n.skip != kUnetNone && add_into(n.skip) != add) return seg_fail(BN_ERR_INVALID, "the graph splits a gradient into a written and a fresh buffer");
        SEG_HIP(seg_dgrad(s, d, geo[i], B, weight(i), G(i), nullptr, dcat, flip));
        SEG_HIP(seg_launch_split(s, dcat, G(n.in), n.skip != kUnetNone ? G(n.skip) : nullptr, B, ca, d.cin - ca, geo[i].hin, geo[i].win, n.upsample, add));
    }
    return BN_OK;
}

int seg_check_run(bn_segtrain *h, int32_t B, int32_t H, int32_t W, const float *colors, const int64_t *targets, float *loss, void *work, size_t bytes)
{
    if (!h || !colors || !targets || !loss || !work) return seg_fail(BN_ERR_INVALID, "null argument");
    if (!seg_shape_ok(B, H, W))
        return seg_fail(BN_ERR_INVALID, "H and W must be multiples of 32 in [32, 2048], num_maps in [1, 4096], num_maps H W <= 2^24, and num_maps "
                                        "(H / 32) (W / 32) > 1 (training needs more than 1 value per channel)");
    if (bytes < seg_plan(h->layers, unet_geometry(h->layers, H, W), B, H, W).total) return seg_fail(BN_ERR_INVALID, "workspace smaller than bn_segtrain_workspace_bytes(num_maps, H, W)");
    return BN_OK;
}

}  // namespace
}  // namespace bn

using bn::seg_fail;

extern "C" {

const char *bn_segtrain_last_error(void) { return bn::g_seg_error.c_str(); }

int64_t bn_segtrain_param_count(int32_t classes)
{
    if (classes < 1 || classes > bn::kUnetMaxClasses) return 0;
    int64_t n = 0;
    bn::seg_host_order(bn::unet_layers(classes), &n);
    return n;
}

int bn_segtrain_create(int32_t device_id, int32_t classes, const float *params_host, int64_t count, bn_segtrain_t **out)
{
    if (!out) return seg_fail(BN_ERR_INVALID, "null handle pointer");
    *out = nullptr;
    if (classes < 1 || classes > bn::kUnetMaxClasses) return seg_fail(BN_ERR_INVALID, "classes must be in [1, " + std::to_string(bn::kUnetMaxClasses) + "]");
    if (!params_host) return seg_fail(BN_ERR_INVALID, "null argument");
    if (count != bn_segtrain_param_count(classes))
        return seg_fail(BN_ERR_INVALID, "count must be bn_segtrain_param_count(classes) = " + std::to_string(bn_segtrain_param_count(classes)));
    for (int64_t i = 0; i < count; ++i)
        if (!std::isfinite(params_host[i])) return seg_fail(BN_ERR_INVALID, "every parameter must be finite (index " + std::to_string(i) + ")");
    if (int rc = bn::seg_open_device(device_id)) return rc;
    BN_ON_DEVICE(seg_fail, device_id);

    bn_segtrain *h = new bn_segtrain();
    h->device = device_id;
    h->classes = classes;
    h->layers = bn::unet_layers(classes);
    int64_t total = 0;
    const std::vector<bn::SegHostSpan> host = bn::seg_host_order(h->layers, &total);
    size_t wt = 0;
    for (int i = 0; i < bn::kUnetConvs; ++i) {
        h->weight_at.push_back((size_t)h->trainable);
        h->trainable += (int64_t)host[i].train;
        h->wt_at.push_back(wt);
        wt += h->layers[i].device_floats();
    }
    for (int i = 0; i < bn::kUnetConvs; ++i) {
        h->stats_at.push_back((size_t)(h->trainable + h->stats));
        h->stats += (int64_t)host[i].stats;
    }
    // the host's order (per convolution: weight, gamma, beta, running mean, running variance) -> the device's (handle header)
    std::vector<float> staged((size_t)count);
    for (int i = 0; i < bn::kUnetConvs; ++i) {
        const bn::SegHostSpan &o = host[i];
        std::memcpy(staged.data() + h->weight_at[i], params_host + o.at, o.train * sizeof(float));
        std::memcpy(staged.data() + h->stats_at[i], params_host + o.at + o.train, o.stats * sizeof(float));
    }
    h->bufs.add(&h->params, (size_t)count * sizeof(float));
    h->bufs.add(&h->grads, (size_t)h->trainable * sizeof(float));
    h->bufs.add(&h->m, (size_t)h->trainable * sizeof(float));
    h->bufs.add(&h->v, (size_t)h->trainable * sizeof(float));
    h->bufs.add(&h->wt, wt * sizeof(float));
    int rc = h->bufs.alloc_all(seg_fail);
    if (rc == BN_OK && hipMemcpy(h->params, staged.data(), (size_t)count * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        rc = seg_fail(BN_ERR_HIP, "the parameter upload failed");
    if (rc != BN_OK) {
        h->bufs.free_all();
        delete h;
        return rc;
    }
    *out = h;
    return BN_OK;
}

void bn_segtrain_destroy(bn_segtrain_t *h)
{
    if (!h) return;
    {
        bn::DeviceGuard guard(h->device);
        h->bufs.free_all();
    }
    delete h;
}

size_t bn_segtrain_workspace_bytes(int32_t num_maps, int32_t H, int32_t W)
{
    if (!bn::seg_shape_ok(num_maps, H, W)) return 0;
    const std::vector<bn::UnetConvDesc> layers = bn::unet_layers(bn::kUnetMaxClasses);
    return bn::seg_plan(layers, bn::unet_geometry(layers, H, W), num_maps, H, W).total;
}

int bn_segtrain_grad_async(bn_segtrain_t *h, void *stream, int32_t num_maps, int32_t H, int32_t W, const float *colors_device,
                           const int64_t *targets_device, float *loss_device, void *workspace_device, size_t workspace_bytes)
{
    if (int rc = bn::seg_check_run(h, num_maps, H, W, colors_device, targets_device, loss_device, workspace_device, workspace_bytes)) return rc;
    BN_ON_DEVICE(seg_fail, h->device);
    return bn::seg_run(h, (hipStream_t)stream, num_maps, H, W, colors_device, targets_device, loss_device, (char *)workspace_device, false);
}

int bn_segtrain_step_async(bn_segtrain_t *h, void *stream, int32_t num_maps, int32_t H, int32_t W, const float *colors_device,
                           const int64_t *targets_device, double lr, double beta1, double beta2, double eps, double weight_decay,
                           float *loss_device, void *workspace_device, size_t workspace_bytes)
{
    if (int rc = bn::seg_check_run(h, num_maps, H, W, colors_device, targets_device, loss_device, workspace_device, workspace_bytes)) return rc;
    if (!bn::seg_adam_ok(lr, beta1, beta2, eps, weight_decay)) return BN_ERR_INVALID;
    BN_ON_DEVICE(seg_fail, h->device);
    if (int rc = bn::seg_run(h, (hipStream_t)stream, num_maps, H, W, colors_device, targets_device, loss_device, (char *)workspace_device, true)) return rc;
    const double t = (double)(h->steps + 1);
    SEG_HIP(bn::seg_launch_adam((hipStream_t)stream, h->params, h->grads, h->m, h->v, h->trainable, lr, beta1, beta2, eps, weight_decay,
                                1.0 - std::pow(beta1, t), std::sqrt(1.0 - std::pow(beta2, t))));
    h->steps += 1;
    return BN_OK;
}

int bn_segtrain_read(bn_segtrain_t *h, int32_t what, float *host, int64_t count)
{
    if (!h || !host) return seg_fail(BN_ERR_INVALID, "null argument");
    if (what < 0 || what > 3) return seg_fail(BN_ERR_INVALID, "what must be 0 (parameters), 1 (gradients), 2 (m) or 3 (v)");
    int64_t total = 0;
    const std::vector<bn::SegHostSpan> order = bn::seg_host_order(h->layers, &total);
    if (count != total) return seg_fail(BN_ERR_INVALID, "count must be bn_segtrain_param_count(classes)");
    BN_ON_DEVICE(seg_fail, h->device);
    SEG_HIP(hipDeviceSynchronize());
    const float *src = what == 0 ? h->params : what == 1 ? h->grads : what == 2 ? h->m : h->v;
    std::vector<float> staged((size_t)(what == 0 ? count : h->trainable));
    SEG_HIP(hipMemcpy(staged.data(), src, staged.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (int i = 0; i < bn::kUnetConvs; ++i) {
        const bn::SegHostSpan &o = order[i];
        std::memcpy(host + o.at, staged.data() + h->weight_at[i], o.train * sizeof(float));
        if (what == 0) std::memcpy(host + o.at + o.train, staged.data() + h->stats_at[i], o.stats * sizeof(float));
        else std::memset(host + o.at + o.train, 0, o.stats * sizeof(float));
    }
    return BN_OK;
}

int64_t bn_segtrain_steps(bn_segtrain_t *h) { return h ? h->steps : -1; }

size_t bn_segtrain_conv2d_backward_workspace_bytes(int32_t num_maps, int32_t cin, int32_t hin, int32_t win, int32_t cout, int32_t ksize, int32_t stride,
                                                   int32_t pad)
{
    if (bn::unet_conv_check(cin, 0, cout, ksize, stride, pad, 0, num_maps, hin, win, true)) return 0;
    const int64_t hout = (hin + 2 * pad - ksize) / stride + 1, wout = (win + 2 * pad - ksize) / stride + 1;
    return bn::unet_align(bn::seg_flip_floats(cin, cout, ksize) * sizeof(float)) + bn::unet_align((size_t)num_maps * cin * hin * win * sizeof(float)) +
           bn::unet_align(bn::seg_partial_floats(num_maps * hout * wout, cout, cin * ksize * ksize) * sizeof(float));
}

int bn_segtrain_conv2d_backward_async(int32_t device_id, void *stream, const float *a_device, int32_t ca, const float *skip_device, int32_t cb,
                                      int32_t upsample, int32_t num_maps, int32_t hin, int32_t win, const float *weights_device, int32_t cout,
                                      int32_t ksize, int32_t stride, int32_t pad, const float *grad_out_device, float *grad_weight_device,
                                      float *grad_a_device, float *grad_skip_device, int32_t accumulate, void *workspace_device, size_t workspace_bytes)
{
    if (!a_device || !weights_device || !grad_out_device || !workspace_device) return seg_fail(BN_ERR_INVALID, "null argument");
    if (cb > 0 && !skip_device) return seg_fail(BN_ERR_INVALID, "cb > 0 needs the skip tensor");
    if (cb == 0 && grad_skip_device) return seg_fail(BN_ERR_INVALID, "a skip gradient needs cb > 0");
    if (const char *why = bn::unet_conv_check(ca, cb, cout, ksize, stride, pad, upsample, num_maps, hin, win, true)) return seg_fail(BN_ERR_INVALID, why);
    const size_t need = bn_segtrain_conv2d_backward_workspace_bytes(num_maps, ca + cb, hin, win, cout, ksize, stride, pad);
    if (workspace_bytes < need) return seg_fail(BN_ERR_INVALID, "workspace smaller than bn_segtrain_conv2d_backward_workspace_bytes(...)");
    if (int rc = bn::seg_open_device(device_id)) return rc;
    BN_ON_DEVICE(seg_fail, device_id);
    hipStream_t s = (hipStream_t)stream;
    const bn::UnetConvDesc d{ca + cb, cout, ksize, stride, pad};
    const bn::UnetGeo geo{hin, win, (hin + 2 * pad - ksize) / stride + 1, (win + 2 * pad - ksize) / stride + 1};
    char *ws = (char *)workspace_device;
    float *flip = (float *)ws;
    float *dcat = (float *)(ws + bn::unet_align(bn::seg_flip_floats(d.cin, cout, ksize) * sizeof(float)));
    float *partial = (float *)((char *)dcat + bn::unet_align((size_t)num_maps * d.cin * hin * win * sizeof(float)));
    if (grad_weight_device) SEG_HIP(bn::seg_wgrad(s, d, geo, num_maps, a_device, ca, skip_device, upsample, grad_out_device, partial, grad_weight_device));
    if (grad_a_device || grad_skip_device) {
        if (!upsample && cb == 0) {
            SEG_HIP(bn::seg_dgrad(s, d, geo, num_maps, weights_device, grad_out_device, accumulate ? grad_a_device : nullptr, grad_a_device, flip));
        } else {
            SEG_HIP(bn::seg_dgrad(s, d, geo, num_maps, weights_device, grad_out_device, nullptr, dcat, flip));
            SEG_HIP(bn::seg_launch_split(s, dcat, grad_a_device, grad_skip_device, num_maps, ca, cb, hin, win, upsample, accumulate ? 1 : 0));
        }
    }
    return BN_OK;
}

int bn_segtrain_batchnorm_forward_async(int32_t device_id, void *stream, const float *x_device, int32_t num_maps, int32_t channels, int64_t cells,
                                        const float *gamma_device, const float *beta_device, const float *residual_device, int32_t relu,
                                        float *running_mean_device, float *running_var_device, float *y_device, double *stats_device)
{
    if (!x_device || !gamma_device || !beta_device || !y_device || !stats_device) return seg_fail(BN_ERR_INVALID, "null argument");
    if (!bn::seg_bn_shape_ok(num_maps, channels, cells)) return BN_ERR_INVALID;
    if (int rc = bn::seg_open_device(device_id)) return rc;
    BN_ON_DEVICE(seg_fail, device_id);
    SEG_HIP(bn::seg_launch_bn_forward((hipStream_t)stream, x_device, gamma_device, beta_device, residual_device, relu ? 1 : 0, running_mean_device,
                                      running_var_device, y_device, stats_device, num_maps, channels, cells));
    return BN_OK;
}

int bn_segtrain_batchnorm_backward_async(int32_t device_id, void *stream, const float *grad_out_device, const float *y_device, const float *x_device,
                                         const double *stats_device, const float *gamma_device, int32_t relu, int32_t num_maps, int32_t channels,
                                         int64_t cells, float *grad_x_device, float *grad_residual_device, float *grad_gamma_device,
                                         float *grad_beta_device, double *sums_device)
{
    if (!grad_out_device || !y_device || !x_device || !stats_device || !gamma_device || !grad_x_device || !grad_gamma_device || !grad_beta_device ||
        !sums_device)
        return seg_fail(BN_ERR_INVALID, "null argument");
    if (!bn::seg_bn_shape_ok(num_maps, channels, cells)) return BN_ERR_INVALID;
    if (int rc = bn::seg_open_device(device_id)) return rc;
    BN_ON_DEVICE(seg_fail, device_id);
    SEG_HIP(bn::seg_launch_bn_backward((hipStream_t)stream, grad_out_device, y_device, x_device, stats_device, gamma_device, relu ? 1 : 0, grad_x_device,
                                       grad_residual_device, grad_gamma_device, grad_beta_device, sums_device, num_maps, channels, cells));
    return BN_OK;
}

int bn_segtrain_maxpool_backward_async(int32_t device_id, void *stream, const float *x_device, const float *grad_out_device, int64_t planes, int32_t hin,
                                       int32_t win, float *grad_x_device, int32_t accumulate)
{
    if (!x_device || !grad_out_device || !grad_x_device) return seg_fail(BN_ERR_INVALID, "null argument");
    if (planes < 1 || hin < 1 || hin > bn::kUnetMaxSide || win < 1 || win > bn::kUnetMaxSide || planes * hin * win > ((int64_t)1 << 30))
        return seg_fail(BN_ERR_INVALID, "planes must be >= 1, the sides in [1, 2048] and planes x hin x win <= 2^30");
    if (int rc = bn::seg_open_device(device_id)) return rc;
    BN_ON_DEVICE(seg_fail, device_id);
    SEG_HIP(bn::seg_launch_maxpool_backward((hipStream_t)stream, x_device, grad_out_device, grad_x_device, planes, hin, win, accumulate ? 1 : 0));
    return BN_OK;
}

int bn_segtrain_cross_entropy_async(int32_t device_id, void *stream, const float *logits_device, const int64_t *targets_device, int32_t num_maps,
                                    int32_t classes, int64_t cells, float *loss_device, float *grad_logits_device, void *workspace_device,
                                    size_t workspace_bytes)
{
    if (!logits_device || !targets_device || !loss_device || !workspace_device) return seg_fail(BN_ERR_INVALID, "null argument");
    if (num_maps < 1 || classes < 1 || classes > bn::kUnetMaxClasses || cells < 1 || num_maps * cells > bn::kUnetMaxPixels)
        return seg_fail(BN_ERR_INVALID, "classes must be in [1, 32] and num_maps x cells in [1, 2^24]");
    if (workspace_bytes < (size_t)(num_maps * cells) * sizeof(double)) return seg_fail(BN_ERR_INVALID, "workspace smaller than 8 bytes per cell");
    if (int rc = bn::seg_open_device(device_id)) return rc;
    BN_ON_DEVICE(seg_fail, device_id);
    SEG_HIP(bn::seg_launch_cross_entropy((hipStream_t)stream, logits_device, targets_device, grad_logits_device, (double *)workspace_device, loss_device,
                                         num_maps, classes, cells));
    return BN_OK;
}

int bn_segtrain_adam_async(int32_t device_id, void *stream, float *params_device, const float *grads_device, float *m_device, float *v_device, int64_t n,
                           int64_t step, double lr, double beta1, double beta2, double eps, double weight_decay)
{
    if (!params_device || !grads_device || !m_device || !v_device) return seg_fail(BN_ERR_INVALID, "null argument");
    if (n < 1 || step < 1) return seg_fail(BN_ERR_INVALID, "n and step must be >= 1");
    if (!bn::seg_adam_ok(lr, beta1, beta2, eps, weight_decay)) return BN_ERR_INVALID;
    if (int rc = bn::seg_open_device(device_id)) return rc;
    BN_ON_DEVICE(seg_fail, device_id);
    SEG_HIP(bn::seg_launch_adam((hipStream_t)stream, params_device, grads_device, m_device, v_device, n, lr, beta1, beta2, eps, weight_decay,
                                1.0 - std::pow(beta1, (double)step), std::sqrt(1.0 - std::pow(beta2, (double)step))));
    return BN_OK;
}

}  // extern "C"
