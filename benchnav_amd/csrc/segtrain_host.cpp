// segtrain_host.cpp -- the C ABI that trains the U-Net terrain classifier (include/benchnav_mppi.h): argument
// checks, the parameter layout, the workspace plan, the launch sequence of one training-mode forward + loss + backward, Adam, and
// the single-layer entry points the layer tests drive.  Kernels: segtrain_kernels.hip and unet_kernels.hip's convolution.
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

size_t seg_align(size_t v) { return (v + 255) & ~(size_t)255; }

// bn_unet_workspace_bytes' range, and more than one value per channel at the bottleneck (BatchNorm in training mode)
bool seg_shape_ok(int64_t num_maps, int64_t H, int64_t W)
{
    return num_maps >= 1 && num_maps <= kUnetMaxMaps && H >= kUnetMinSide && H <= kUnetMaxSide && W >= kUnetMinSide && W <= kUnetMaxSide &&
           H % 32 == 0 && W % 32 == 0 && num_maps * H * W <= kUnetMaxPixels && num_maps * (H / 32) * (W / 32) > 1;
}

constexpr int kFirst[4] = {kUnetLayer1, kUnetLayer2, kUnetLayer3, kUnetLayer4};
constexpr int kLayerOut[4] = {4, 9, 14, 19};             // the table index of each encoder layer's last convolution
constexpr int kSkipOf[5] = {14, 9, 4, 0, -1};            // the convolution whose output a decoder block concatenates
constexpr int kDecIn[5] = {512, 256, 128, 64, 32}, kDecSkip[5] = {256, 128, 64, 64, 0};

struct SegGeo { int hin, win, hout, wout; };

// the (virtual) input and the output size of every convolution of the table
std::vector<SegGeo> seg_geometry(int H, int W)
{
    std::vector<SegGeo> g(kUnetConvs);
    g[0] = {H, W, H / 2, W / 2};
    for (int l = 0; l < 4; ++l) {
        const int ho = H >> (2 + l), wo = W >> (2 + l), hi = l ? ho * 2 : ho, wi = l ? wo * 2 : wo, i = kFirst[l], n = l ? 5 : 4;
        for (int j = 0; j < n; ++j) g[i + j] = {ho, wo, ho, wo};
        g[i] = {hi, wi, ho, wo};
        if (l) g[i + 2] = {hi, wi, ho, wo};
    }
    for (int b = 0; b < 5; ++b) g[kUnetDecoder + 2 * b] = g[kUnetDecoder + 2 * b + 1] = {H >> (4 - b), W >> (4 - b), H >> (4 - b), W >> (4 - b)};
    g[kUnetHead] = {H, W, H, W};
    return g;
}

size_t seg_flip_floats(int cin, int cout, int ksize)
{
    const size_t cinpad = unet_round_up(cin, kUnetTile);
    return (size_t)unet_round_up(cout * ksize * ksize, kUnetKStep) * cinpad + cinpad;
}

size_t seg_partial_floats(int64_t npix, int cout, int k) { return (size_t)seg_split(npix, cout, k).chunks * cout * k; }

// Where everything one step keeps lives in the workspace (byte offsets, multiples of 256): per convolution its raw output c, the
// activation y behind BatchNorm and the gradient g (of y, then in place of c), and the batch statistics as float64.
struct SegPlan {
    size_t c[kUnetConvs] = {}, y[kUnetConvs] = {}, g[kUnetConvs] = {}, stats[kUnetConvs] = {};
    size_t pool = 0, gpool = 0, logits = 0, dlogits = 0, dcat = 0, flip = 0, partial = 0, sums = 0, terms = 0, total = 0;
};

SegPlan seg_plan(const std::vector<UnetConvDesc> &layers, int64_t n, int H, int W)
{
    SegPlan p;
    const std::vector<SegGeo> geo = seg_geometry(H, W);
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t o = at;
        at += seg_align(bytes);
        return o;
    };
    size_t flip = 0, partial = 0;
    for (int i = 0; i < kUnetConvs; ++i) {
        const UnetConvDesc &d = layers[i];
        const size_t act = (size_t)(n * d.cout * geo[i].hout * geo[i].wout) * sizeof(float);
        if (i < kUnetHead) {
            p.c[i] = take(act);
            p.y[i] = take(act);
            p.g[i] = take(act);
            p.stats[i] = take((size_t)2 * d.cout * sizeof(double));
        }
        if (i) flip = std::max(flip, seg_flip_floats(d.cin, d.cout, d.ksize));
        partial = std::max(partial, seg_partial_floats(n * geo[i].hout * geo[i].wout, d.cout, d.K()));
    }
    p.pool = take((size_t)(n * 64 * (H / 4) * (W / 4)) * sizeof(float));
    p.gpool = take((size_t)(n * 64 * (H / 4) * (W / 4)) * sizeof(float));
    p.logits = take((size_t)(n * kUnetMaxClasses * H * W) * sizeof(float));
    p.dlogits = take((size_t)(n * kUnetMaxClasses * H * W) * sizeof(float));
    size_t dcat = 0;
    for (int b = 0; b < 5; ++b) dcat = std::max(dcat, (size_t)(n * (kDecIn[b] + kDecSkip[b]) * (H >> (4 - b)) * (W >> (4 - b))));
    p.dcat = take(dcat * sizeof(float));
    p.flip = take(flip * sizeof(float));
    p.partial = take(partial * sizeof(float));
    p.sums = take((size_t)2 * 512 * sizeof(double));
    p.terms = take((size_t)(n * H * W) * sizeof(double));
    p.total = at;
    return p;
}

int seg_open_device(int32_t device_id) { return open_device(device_id, seg_fail); }

int64_t seg_host_floats(const UnetConvDesc &d, bool head) { return (int64_t)d.cout * d.K() + (head ? d.cout : 4 * d.cout); }

// dX = backward-data of one convolution into `out` (num_maps, cin, hin, win), plus `residual` where given: stride 1 through the
// forward convolution on the flipped weight, stride 2 through the strided kernel.  `flip` is scratch for that weight.
hipError_t seg_dgrad(hipStream_t s, const float *w, const float *dy, int num_maps, int cin, int cout, int ksize, int stride, int pad, const SegGeo &geo,
                     const float *residual, float *out, float *flip)
{
    const int k = cout * ksize * ksize, kpad = unet_round_up(k, kUnetKStep), cinpad = unet_round_up(cin, kUnetTile);
    float *zero_bias = flip + (size_t)kpad * cinpad;
    if (hipError_t e = seg_launch_flip(s, w, flip, zero_bias, cout, cin, ksize, kpad, cinpad)) return e;
    if (stride == 1) {
        UnetConvArgs g{};
        g.a = dy; g.b = nullptr; g.wt = flip; g.bias = zero_bias; g.residual = residual; g.out = out;
        g.num_maps = num_maps; g.ca = cout; g.cb = 0; g.hin = geo.hout; g.win = geo.wout; g.hout = geo.hin; g.wout = geo.win;
        g.cout = cin; g.coutpad = cinpad; g.k = k; g.kpad = kpad; g.stride = 1; g.pad = ksize - 1 - pad; g.upsample = 0; g.relu = 0;
        return unet_launch_conv(s, ksize, g);
    }
    SegConvGrad g{};
    g.dy = dy; g.wt = flip; g.residual = residual; g.out = out;
    g.num_maps = num_maps; g.ca = cin; g.cb = 0; g.hin = geo.hin; g.win = geo.win; g.hout = geo.hout; g.wout = geo.wout;
    g.cout = cout; g.k = k; g.kpad = kpad; g.cinpad = cinpad; g.stride = stride; g.pad = pad;
    return seg_launch_dgrad_strided(s, ksize, g);
}

// dW = backward-weight of one convolution: the partial sums into `partial`, then their sum in ascending chunk order into dw
hipError_t seg_wgrad(hipStream_t s, const float *a, int ca, const float *b, int cb, int upsample, const float *dy, int num_maps, int cout, int ksize,
                     int stride, int pad, const SegGeo &geo, float *partial, float *dw)
{
    SegConvGrad g{};
    g.a = a; g.b = b; g.dy = dy; g.out = partial;
    g.num_maps = num_maps; g.ca = ca; g.cb = cb; g.hin = geo.hin; g.win = geo.win; g.hout = geo.hout; g.wout = geo.wout;
    g.cout = cout; g.k = (ca + cb) * ksize * ksize; g.stride = stride; g.pad = pad; g.upsample = upsample;
    const SegSplit sp = seg_split((int64_t)num_maps * geo.hout * geo.wout, cout, g.k);
    g.chunks = sp.chunks; g.stages = sp.stages;
    if (hipError_t e = seg_launch_wgrad(s, ksize, g)) return e;
    return seg_launch_wgrad_reduce(s, partial, dw, (int64_t)cout * g.k, sp.chunks);
}

struct SegInput { const float *a; int ca; const float *b; int cb; int upsample; };

// One training-mode forward, the loss and the backward on `s`; the gradients end in h->grads.
int seg_run(bn_segtrain *h, hipStream_t s, int B, int H, int W, const float *colors, const int64_t *targets, float *loss, char *ws, bool update_stats)
{
    const SegPlan p = seg_plan(h->layers, B, H, W);
    const std::vector<SegGeo> geo = seg_geometry(H, W);
    auto C = [&](int i) { return (float *)(ws + p.c[i]); };
    auto Y = [&](int i) { return (float *)(ws + p.y[i]); };
    auto G = [&](int i) { return (float *)(ws + p.g[i]); };
    float *pool = (float *)(ws + p.pool), *gpool = (float *)(ws + p.gpool), *logits = (float *)(ws + p.logits), *dlogits = (float *)(ws + p.dlogits);
    float *dcat = (float *)(ws + p.dcat), *flip = (float *)(ws + p.flip), *partial = (float *)(ws + p.partial);
    double *sums = (double *)(ws + p.sums), *terms = (double *)(ws + p.terms);
    auto weight = [&](int i) { return h->params + h->weight_at[i]; };
    auto gamma = [&](int i) { return weight(i) + (size_t)h->layers[i].cout * h->layers[i].K(); };
    auto wgrad_at = [&](int i) { return h->grads + h->weight_at[i]; };
    SegInput in[kUnetConvs];

    // the forward reads the weights as unet_conv_kernel does: re-laid from the current parameters, a zero bias except the head's
    for (int i = 0; i < kUnetConvs; ++i) {
        const UnetConvDesc &d = h->layers[i];
        float *wt = h->wt + h->wt_at[i];
        SEG_HIP(unet_launch_relayout(s, weight(i), i == kUnetHead ? gamma(i) : nullptr, wt, wt + (size_t)d.kpad() * d.coutpad(), d.cout, d.K(), d.kpad(),
                                     d.coutpad()));
    }
    auto conv = [&](int i, const float *a, int ca, const float *b, int cb, int upsample, float *out) -> hipError_t {
        const UnetConvDesc &d = h->layers[i];
        in[i] = SegInput{a, ca, b, cb, upsample};
        UnetConvArgs g{};
        g.a = a; g.b = b;
        g.wt = h->wt + h->wt_at[i];
        g.bias = g.wt + (size_t)d.kpad() * d.coutpad();
        g.out = out;
        g.num_maps = B; g.ca = ca; g.cb = cb; g.hin = geo[i].hin; g.win = geo[i].win; g.hout = geo[i].hout; g.wout = geo[i].wout;
        g.cout = d.cout; g.coutpad = d.coutpad(); g.k = d.K(); g.kpad = d.kpad(); g.stride = d.stride; g.pad = d.pad; g.upsample = upsample;
        return unet_launch_conv(s, d.ksize, g);
    };
    auto bn = [&](int i, const float *residual, int relu) -> hipError_t {
        const int cout = h->layers[i].cout;
        float *rm = update_stats ? h->params + h->stats_at[i] : nullptr;
        return seg_launch_bn_forward(s, C(i), gamma(i), gamma(i) + cout, residual, relu, rm, rm ? rm + cout : nullptr, Y(i), (double *)(ws + p.stats[i]), B,
                                     cout, (int64_t)geo[i].hout * geo[i].wout);
    };
    auto layer = [&](int i, const float *a, int ca, const float *residual, int relu) -> hipError_t {
        if (hipError_t e = conv(i, a, ca, nullptr, 0, 0, C(i))) return e;
        return bn(i, residual, relu);
    };

    SEG_HIP(layer(0, colors, 3, nullptr, 1));
    SEG_HIP(unet_launch_maxpool(s, Y(0), pool, (int64_t)B * 64, H / 2, W / 2, H / 4, W / 4));
    const float *x = pool;
    int cin = 64;
    for (int l = 0; l < 4; ++l) {
        const int w = h->layers[kFirst[l]].cout, i = kFirst[l], j = l ? i + 3 : i + 2;
        const float *identity = x;
        SEG_HIP(layer(i, x, cin, nullptr, 1));
        if (l) {
            SEG_HIP(layer(i + 2, x, cin, nullptr, 0));
            identity = Y(i + 2);
        }
        SEG_HIP(layer(i + 1, Y(i), w, identity, 1));
        SEG_HIP(layer(j, Y(i + 1), w, nullptr, 1));
        SEG_HIP(layer(j + 1, Y(j), w, Y(i + 1), 1));
        x = Y(j + 1);
        cin = w;
    }
    for (int b = 0; b < 5; ++b) {
        const int i = kUnetDecoder + 2 * b;
        SEG_HIP(conv(i, x, kDecIn[b], kDecSkip[b] ? Y(kSkipOf[b]) : nullptr, kDecSkip[b], 1, C(i)));
        SEG_HIP(bn(i, nullptr, 1));
        SEG_HIP(layer(i + 1, Y(i), h->layers[i].cout, nullptr, 1));
        x = Y(i + 1);
    }
    SEG_HIP(conv(kUnetHead, x, 16, nullptr, 0, 0, logits));
    SEG_HIP(seg_launch_cross_entropy(s, logits, targets, dlogits, terms, loss, B, h->classes, (int64_t)H * W));

    // ---- backward ----
    auto bn_back = [&](int i, int relu, float *dres) -> hipError_t {
        const int cout = h->layers[i].cout;
        float *dgamma = wgrad_at(i) + (size_t)cout * h->layers[i].K();
        return seg_launch_bn_backward(s, G(i), Y(i), C(i), (const double *)(ws + p.stats[i]), gamma(i), relu, G(i), dres, dgamma, dgamma + cout, sums, B,
                                      cout, (int64_t)geo[i].hout * geo[i].wout);
    };
    auto wgrad = [&](int i, const float *dy) -> hipError_t {
        const UnetConvDesc &d = h->layers[i];
        return seg_wgrad(s, in[i].a, in[i].ca, in[i].b, in[i].cb, in[i].upsample, dy, B, d.cout, d.ksize, d.stride, d.pad, geo[i], partial, wgrad_at(i));
    };
    auto dgrad = [&](int i, const float *dy, const float *residual, float *out) -> hipError_t {
        const UnetConvDesc &d = h->layers[i];
        return seg_dgrad(s, weight(i), dy, B, d.cin, d.cout, d.ksize, d.stride, d.pad, geo[i], residual, out, flip);
    };
    // BatchNorm's backward in place, the weight gradient, and the data gradient into `out` (added to what is there if `add`)
    auto back = [&](int i, int relu, float *dres, float *out, bool add) -> hipError_t {
        if (hipError_t e = bn_back(i, relu, dres)) return e;
        if (hipError_t e = wgrad(i, G(i))) return e;
        return out ? dgrad(i, G(i), add ? out : nullptr, out) : hipSuccess;
    };

    SEG_HIP(wgrad(kUnetHead, dlogits));
    SEG_HIP(seg_launch_bias_grad(s, dlogits, wgrad_at(kUnetHead) + (size_t)h->classes * h->layers[kUnetHead].K(), B, h->classes, (int64_t)H * W));
    SEG_HIP(dgrad(kUnetHead, dlogits, nullptr, G(29)));
    for (int b = 4; b >= 0; --b) {
        const int i = kUnetDecoder + 2 * b;
        SEG_HIP(back(i + 1, 1, nullptr, G(i), false));
        SEG_HIP(back(i, 1, nullptr, dcat, false));
        SEG_HIP(seg_launch_split(s, dcat, b ? G(i - 1) : G(kLayerOut[3]), kDecSkip[b] ? G(kSkipOf[b]) : nullptr, B, kDecIn[b], kDecSkip[b], geo[i].hin,
                                 geo[i].win, 1, 0));
    }
    for (int l = 3; l >= 0; --l) {
        const int i = kFirst[l], j = l ? i + 3 : i + 2;
        float *gx = l ? G(kLayerOut[l - 1]) : gpool;     // layers 2-4: the decoder's skip gradient is there already
        SEG_HIP(back(j + 1, 1, G(i + 1), G(j), false));
        SEG_HIP(back(j, 1, nullptr, G(i + 1), true));
        SEG_HIP(back(i + 1, 1, l ? G(i + 2) : gpool, G(i), false));
        SEG_HIP(back(i, 1, nullptr, gx, true));
        if (l) SEG_HIP(back(i + 2, 0, nullptr, gx, true));
    }
    SEG_HIP(seg_launch_maxpool_backward(s, Y(0), gpool, G(0), (int64_t)B * 64, H / 2, W / 2, 1));
    SEG_HIP(back(0, 1, nullptr, nullptr, false));
    return BN_OK;
}

int seg_check_run(bn_segtrain *h, int32_t B, int32_t H, int32_t W, const float *colors, const int64_t *targets, float *loss, void *work, size_t bytes)
{
    if (!h || !colors || !targets || !loss || !work) return seg_fail(BN_ERR_INVALID, "null argument");
    if (!seg_shape_ok(B, H, W))
        return seg_fail(BN_ERR_INVALID, "H and W must be multiples of 32 in [32, 2048], num_maps in [1, 4096], num_maps H W <= 2^24, and num_maps "
                                        "(H / 32) (W / 32) > 1 (training needs more than 1 value per channel)");
    if (bytes < seg_plan(h->layers, B, H, W).total) return seg_fail(BN_ERR_INVALID, "workspace smaller than bn_segtrain_workspace_bytes(num_maps, H, W)");
    return BN_OK;
}

// checks shared by the single-layer entry points
bool seg_conv_ok(int ca, int cb, int cout, int ksize, int stride, int pad, int upsample, int num_maps, int hin, int win, std::string *why)
{
    if (ca < 1 || cb < 0 || ca + cb > 4096 || cout < 1 || cout > 4096) *why = "channels must be in [1, 4096]";
    else if (ksize != 1 && ksize != 3 && ksize != 7) *why = "ksize must be 1, 3 or 7";
    else if (stride < 1 || stride > 2 || pad < 0 || pad > 3 || pad > ksize - 1) *why = "stride must be 1 or 2 and pad in [0, min(3, ksize - 1)]";
    else if (upsample != 0 && upsample != 1) *why = "upsample must be 0 or 1";
    else if (num_maps < 1 || num_maps > kUnetMaxMaps || hin < 1 || hin > kUnetMaxSide || win < 1 || win > kUnetMaxSide) *why = "num_maps must be in [1, 4096] and the input sides in [1, 2048]";
    else if (upsample && ((hin | win) & 1)) *why = "an upsampled input has even sides";
    else if (hin + 2 * pad < ksize || win + 2 * pad < ksize) *why = "the kernel does not fit the padded input";
    else {
        const int64_t hout = (hin + 2 * pad - ksize) / stride + 1, wout = (win + 2 * pad - ksize) / stride + 1;
        if ((int64_t)num_maps * hin * win > kUnetMaxPixels || num_maps * hout * wout > kUnetMaxPixels) *why = "num_maps x pixels must be <= 2^24";
        else if ((int64_t)num_maps * (ca + cb) * hin * win >= ((int64_t)1 << 31) || num_maps * cout * hout * wout >= ((int64_t)1 << 31)) *why = "a tensor must hold fewer than 2^31 elements";
        else return true;
    }
    return false;
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
    const std::vector<bn::UnetConvDesc> layers = bn::unet_layers(classes);
    for (int i = 0; i < bn::kUnetConvs; ++i) n += bn::seg_host_floats(layers[i], i == bn::kUnetHead);
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
    size_t wt = 0;
    for (int i = 0; i < bn::kUnetConvs; ++i) {
        const bn::UnetConvDesc &d = h->layers[i];
        h->weight_at.push_back((size_t)h->trainable);
        h->trainable += (int64_t)d.cout * d.K() + (i == bn::kUnetHead ? d.cout : 2 * d.cout);
        h->wt_at.push_back(wt);
        wt += d.device_floats();
    }
    for (int i = 0; i < bn::kUnetConvs; ++i) {
        h->stats_at.push_back((size_t)(h->trainable + h->stats));
        if (i != bn::kUnetHead) h->stats += 2 * h->layers[i].cout;
    }
    // the host's order (per convolution: weight, gamma, beta, running mean, running variance) -> the device's (handle header)
    std::vector<float> staged((size_t)count);
    size_t at = 0;
    for (int i = 0; i < bn::kUnetConvs; ++i) {
        const bn::UnetConvDesc &d = h->layers[i];
        const size_t train = (size_t)d.cout * d.K() + (i == bn::kUnetHead ? d.cout : 2 * d.cout);
        std::memcpy(&staged[h->weight_at[i]], params_host + at, train * sizeof(float));
        if (i != bn::kUnetHead) std::memcpy(&staged[h->stats_at[i]], params_host + at + train, (size_t)2 * d.cout * sizeof(float));
        at += (size_t)bn::seg_host_floats(d, i == bn::kUnetHead);
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
    return bn::seg_plan(bn::unet_layers(bn::kUnetMaxClasses), num_maps, H, W).total;
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
    if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !(weight_decay >= 0.0) || !std::isfinite(lr) ||
        !std::isfinite(eps) || !std::isfinite(weight_decay))
        return seg_fail(BN_ERR_INVALID, "lr, eps and weight_decay must be finite and >= 0, beta1 and beta2 in [0, 1)");
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
    if (count != bn_segtrain_param_count(h->classes)) return seg_fail(BN_ERR_INVALID, "count must be bn_segtrain_param_count(classes)");
    BN_ON_DEVICE(seg_fail, h->device);
    SEG_HIP(hipDeviceSynchronize());
    const float *src = what == 0 ? h->params : what == 1 ? h->grads : what == 2 ? h->m : h->v;
    std::vector<float> staged((size_t)(what == 0 ? count : h->trainable));
    SEG_HIP(hipMemcpy(staged.data(), src, staged.size() * sizeof(float), hipMemcpyDeviceToHost));
    size_t at = 0;
    for (int i = 0; i < bn::kUnetConvs; ++i) {
        const bn::UnetConvDesc &d = h->layers[i];
        const bool head = i == bn::kUnetHead;
        const size_t train = (size_t)d.cout * d.K() + (head ? d.cout : 2 * d.cout);
        std::memcpy(host + at, &staged[h->weight_at[i]], train * sizeof(float));
        if (!head) {
            if (what == 0) std::memcpy(host + at + train, &staged[h->stats_at[i]], (size_t)2 * d.cout * sizeof(float));
            else std::memset(host + at + train, 0, (size_t)2 * d.cout * sizeof(float));
        }
        at += (size_t)bn::seg_host_floats(d, head);
    }
    return BN_OK;
}

int64_t bn_segtrain_steps(bn_segtrain_t *h) { return h ? h->steps : -1; }

size_t bn_segtrain_conv2d_backward_workspace_bytes(int32_t num_maps, int32_t cin, int32_t hin, int32_t win, int32_t cout, int32_t ksize, int32_t stride,
                                                   int32_t pad)
{
    std::string why;
    if (!bn::seg_conv_ok(cin, 0, cout, ksize, stride, pad, 0, num_maps, hin, win, &why)) return 0;
    const int64_t hout = (hin + 2 * pad - ksize) / stride + 1, wout = (win + 2 * pad - ksize) / stride + 1;
    return bn::seg_align(bn::seg_flip_floats(cin, cout, ksize) * sizeof(float)) + bn::seg_align((size_t)num_maps * cin * hin * win * sizeof(float)) +
           bn::seg_align(bn::seg_partial_floats(num_maps * hout * wout, cout, cin * ksize * ksize) * sizeof(float));
}

int bn_segtrain_conv2d_backward_async(int32_t device_id, void *stream, const float *a_device, int32_t ca, const float *skip_device, int32_t cb,
                                      int32_t upsample, int32_t num_maps, int32_t hin, int32_t win, const float *weights_device, int32_t cout,
                                      int32_t ksize, int32_t stride, int32_t pad, const float *grad_out_device, float *grad_weight_device,
                                      float *grad_a_device, float *grad_skip_device, int32_t accumulate, void *workspace_device, size_t workspace_bytes)
{
    if (!a_device || !weights_device || !grad_out_device || !workspace_device) return seg_fail(BN_ERR_INVALID, "null argument");
    if (cb > 0 && !skip_device) return seg_fail(BN_ERR_INVALID, "cb > 0 needs the skip tensor");
    if (cb == 0 && grad_skip_device) return seg_fail(BN_ERR_INVALID, "a skip gradient needs cb > 0");
    std::string why;
    if (!bn::seg_conv_ok(ca, cb, cout, ksize, stride, pad, upsample, num_maps, hin, win, &why)) return seg_fail(BN_ERR_INVALID, why);
    const size_t need = bn_segtrain_conv2d_backward_workspace_bytes(num_maps, ca + cb, hin, win, cout, ksize, stride, pad);
    if (workspace_bytes < need) return seg_fail(BN_ERR_INVALID, "workspace smaller than bn_segtrain_conv2d_backward_workspace_bytes(...)");
    if (int rc = bn::seg_open_device(device_id)) return rc;
    BN_ON_DEVICE(seg_fail, device_id);
    hipStream_t s = (hipStream_t)stream;
    const int cin = ca + cb;
    const bn::SegGeo geo{hin, win, (hin + 2 * pad - ksize) / stride + 1, (win + 2 * pad - ksize) / stride + 1};
    char *ws = (char *)workspace_device;
    float *flip = (float *)ws;
    float *dcat = (float *)(ws + bn::seg_align(bn::seg_flip_floats(cin, cout, ksize) * sizeof(float)));
    float *partial = (float *)((char *)dcat + bn::seg_align((size_t)num_maps * cin * hin * win * sizeof(float)));
    if (grad_weight_device)
        SEG_HIP(bn::seg_wgrad(s, a_device, ca, skip_device, cb, upsample, grad_out_device, num_maps, cout, ksize, stride, pad, geo, partial, grad_weight_device));
    if (grad_a_device || grad_skip_device) {
        if (!upsample && cb == 0) {
            SEG_HIP(bn::seg_dgrad(s, weights_device, grad_out_device, num_maps, cin, cout, ksize, stride, pad, geo, accumulate ? grad_a_device : nullptr,
                                  grad_a_device, flip));
        } else {
            SEG_HIP(bn::seg_dgrad(s, weights_device, grad_out_device, num_maps, cin, cout, ksize, stride, pad, geo, nullptr, dcat, flip));
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
    if (num_maps < 1 || channels < 1 || channels > 4096 || cells < 1 || num_maps * cells > bn::kUnetMaxPixels || num_maps * cells < 2 ||
        num_maps * cells * channels >= ((int64_t)1 << 31))
        return seg_fail(BN_ERR_INVALID, "channels must be in [1, 4096], num_maps x cells in [2, 2^24] (more than 1 value per channel), the tensor < 2^31");
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
    if (num_maps < 1 || channels < 1 || channels > 4096 || cells < 1 || num_maps * cells > bn::kUnetMaxPixels || num_maps * cells < 2 ||
        num_maps * cells * channels >= ((int64_t)1 << 31))
        return seg_fail(BN_ERR_INVALID, "channels must be in [1, 4096], num_maps x cells in [2, 2^24], the tensor < 2^31");
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
    if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !(weight_decay >= 0.0) || !std::isfinite(lr) ||
        !std::isfinite(eps) || !std::isfinite(weight_decay))
        return seg_fail(BN_ERR_INVALID, "lr, eps and weight_decay must be finite and >= 0, beta1 and beta2 in [0, 1)");
    if (int rc = bn::seg_open_device(device_id)) return rc;
    BN_ON_DEVICE(seg_fail, device_id);
    SEG_HIP(bn::seg_launch_adam((hipStream_t)stream, params_device, grads_device, m_device, v_device, n, lr, beta1, beta2, eps, weight_decay,
                                1.0 - std::pow(beta1, (double)step), std::sqrt(1.0 - std::pow(beta2, (double)step))));
    return BN_OK;
}

}  // extern "C"
