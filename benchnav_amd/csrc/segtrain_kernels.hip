// segtrain_kernels.hip -- the kernels that train the U-Net terrain classifier: convolution backward-weight and the
// strided backward-data on the exact float32 MFMA, BatchNorm in training mode (forward and backward), the max-pool's backward, the
// cross-entropy and Adam.  Host side: segtrain_host.cpp, shared types: segtrain_handle.h.  The forward convolution and the stride-1
// backward-data are unet_kernels.hip's convolution, launched with other operands.
//
// Backward-weight is the GEMM  dW[co][k] = sum_pixel dY[co][pixel] * X[k][pixel]  with the forward's k = ci ks^2 + ky ks + kx and the
// forward's gather (upsample + concat, stride, zero padding).  A workgroup of four waves owns 64 output channels x 64 k and one
// chunk of the pixel axis; wave w owns channels 16 w ... 16 w + 15 as four 16 x 16 accumulators.  Per stage 64 pixels of both
// operands go through LDS as [channel or k][pixel] (global reads run along the pixels; row pitch 66 floats: the 16 rows x 4 pixels
// of a fragment read fall on 32 different banks per half wave), the next stage is in flight in registers meanwhile.
//
// Summation orders (two runs from the same state give the same bits; no atomics anywhere):
//   backward-weight: a partial is the sum over slabs of 128 consecutive pixels of one pixel-ordered fmaf chain each, the slabs added
//     in ascending order; segtrain_wgrad_reduce_kernel adds the partials in ascending chunk order.  seg_split() (segtrain_handle.h)
//     fixes the partition from the shape alone.
//   backward-data, strided: the forward convolution's own order (slabs of 128 consecutive k, ascending).
//   per-channel and whole-tensor reductions: float64; thread t adds elements t, t + 256, ... in ascending order, then a binary tree
//     over the 256 threads.  Elementwise arithmetic: float64 from the float32 operands, rounded once.
#include "segtrain_handle.h"
#include "unet_conv_tile.h"

namespace bn {
namespace {

template <int KS>
__global__ __launch_bounds__(256) void segtrain_wgrad_kernel(const SegConvGrad p)
{
    __shared__ float As[kUnetTile * kSegPitch], Bs[kUnetTile * kSegPitch];
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int k0 = blockIdx.x * kUnetTile, co0 = blockIdx.y * kUnetTile, chunk = blockIdx.z;
    const int cells = p.hout * p.wout, npix = cells * p.num_maps;            // num_maps x pixels <= 2^24 (checked on the host)
    const int plane_a = p.upsample ? (p.hin >> 1) * (p.win >> 1) : p.hin * p.win;
    const int total = (npix + kUnetTile - 1) / kUnetTile, first = chunk * p.stages, count = min(p.stages, total - first);
    const bool active = co0 + wave * 16 < p.cout;

    float ra[kRows], rb[kRows];
    auto load = [&](int stage) {             // rows wave, wave + 4, ... of both operands at this lane's pixel of the stage
        const int pix = (first + stage) * kUnetTile + lane;
        const bool valid = pix < npix;
        int map = 0, rem = 0, iy0 = 0, ix0 = 0;
        if (valid) {
            map = pix / cells;
            rem = pix - map * cells;
            const int oy = rem / p.wout;
            iy0 = oy * p.stride - p.pad;
            ix0 = (rem - oy * p.wout) * p.stride - p.pad;
        }
        const float *map_a = p.a + (int64_t)map * p.ca * plane_a, *map_b = p.b + (int64_t)map * p.cb * (p.hin * p.win);
        const float *dy = p.dy + (int64_t)map * p.cout * cells + rem;
        // The 16 rows' k are the same in every stage; left visible, the compiler keeps all their decoded taps in scalar registers
        // across the loop and spills them.  `again` is 0 (a stage index is below 2^18) but not to the compiler: the taps are decoded
        // per stage on the scalar unit, as in the forward convolution.
        const int again = (first + stage) >> 20;
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
            const int r = wave + 4 * j + again;
            ra[j] = (valid && co0 + r < p.cout) ? dy[(int64_t)(co0 + r) * cells] : 0.0f;
            rb[j] = unet_gather<KS>(p, k0 + r, valid, map_a, map_b, iy0, ix0);
        }
    };
    load(0);
    f32x4 acc[4], tot[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) { acc[n] = f32x4{0.f, 0.f, 0.f, 0.f}; tot[n] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    const int frow = lane >> 4, fcol = lane & 15;
    for (int s = 0; s < count; ++s) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
            As[(wave + 4 * j) * kSegPitch + lane] = ra[j];
            Bs[(wave + 4 * j) * kSegPitch + lane] = rb[j];
        }
        __syncthreads();
        if (s + 1 < count) load(s + 1);
        if (active) {
#pragma unroll
            for (int q = 0; q < kUnetTile / 4; ++q) {    // four pixels: one MFMA step of each accumulator
                const float a = As[(wave * 16 + fcol) * kSegPitch + q * 4 + frow];
#pragma unroll
                for (int n = 0; n < 4; ++n)
                    acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Bs[(n * 16 + fcol) * kSegPitch + q * 4 + frow], acc[n], 0, 0, 0);
            }
            if ((s & (kSlabStages - 1)) == kSlabStages - 1) {
#pragma unroll
                for (int n = 0; n < 4; ++n) { tot[n] += acc[n]; acc[n] = f32x4{0.f, 0.f, 0.f, 0.f}; }
            }
        }
    }
    if (!active) return;
    if (count & (kSlabStages - 1)) {
#pragma unroll
        for (int n = 0; n < 4; ++n) tot[n] += acc[n];
    }
    // C/D map: column (k) = lane & 15, row (channel) = 4 (lane >> 4) + register
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int k = k0 + n * 16 + fcol;
        if (k >= p.k) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int co = co0 + wave * 16 + 4 * frow + r;
            if (co < p.cout) p.out[((int64_t)chunk * p.cout + co) * p.k + k] = tot[n][r];
        }
    }
}

__global__ __launch_bounds__(256) void segtrain_wgrad_reduce_kernel(const float *partial, float *dw, int64_t n, int chunks)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = partial[i];
    for (int c = 1; c < chunks; ++c) s += partial[c * n + i];
    dw[i] = s;
}

// Backward-data of a strided convolution as a forward convolution over dY spread out by the stride: row k = (co, ty, tx) of the
// flipped weight meets dY[co][(iy + pad - ky) / stride][...] with ky = ks - 1 - ty, where that division is exact and in range.
template <int KS>
__device__ __forceinline__ float seg_gather_dy(const SegConvGrad &p, int k, bool pixel_valid, const float *map_dy, int py0, int px0)
{
    const int co = k / (KS * KS), tap = k - co * (KS * KS), ty = tap / KS, tx = tap - ty * KS;
    const int py = py0 + ty, px = px0 + tx, sh = p.stride - 1;               // stride 1 or 2
    if (!pixel_valid || k >= p.k || py < 0 || px < 0 || ((py | px) & sh)) return 0.0f;
    const int oy = py >> sh, ox = px >> sh;
    if (oy >= p.hout || ox >= p.wout) return 0.0f;
    return map_dy[co * (p.hout * p.wout) + oy * p.wout + ox];
}

// The forward convolution's tiling and summation order (unet_kernels.hip) with the gather above: 64 input channels x 64 input
// cells per workgroup, k = co ks^2 + tap over the output channels.
template <int KS>
__global__ __launch_bounds__(256) void segtrain_dgrad_kernel(const SegConvGrad p)
{
    __shared__ float As[kStage * kPitch], Bs[kStage * kPitch];
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int col = lane, row0 = wave, cin = p.ca + p.cb;
    const int cells = p.hin * p.win, npix = cells * p.num_maps;
    const int pix = blockIdx.x * kUnetTile + col;
    const bool pixel_valid = pix < npix;
    int map = 0, py0 = 0, px0 = 0;
    if (pixel_valid) {
        map = pix / cells;
        const int rem = pix - map * cells, iy = rem / p.win;
        py0 = iy - (KS - 1 - p.pad);
        px0 = (rem - iy * p.win) - (KS - 1 - p.pad);
    }
    const float *map_dy = p.dy + (int64_t)map * p.cout * (p.hout * p.wout);
    const int ci0 = blockIdx.y * kUnetTile;
    const float *wcol = p.wt + ci0 + col;
    const bool active = ci0 + wave * 16 < cin;

    float ra[kRows], rb[kRows];
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
        const int k = row0 + 4 * j;
        ra[j] = k < p.kpad ? wcol[(size_t)k * p.cinpad] : 0.0f;
        rb[j] = seg_gather_dy<KS>(p, k, pixel_valid, map_dy, py0, px0);
    }
    f32x4 acc[4], tot[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) { acc[n] = f32x4{0.f, 0.f, 0.f, 0.f}; tot[n] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    const int frow = lane >> 4, fcol = lane & 15;
    int step = 0;
    for (int k0 = 0; k0 < p.kpad; k0 += kStage, ++step) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
            As[(row0 + 4 * j) * kPitch + col] = ra[j];
            Bs[(row0 + 4 * j) * kPitch + col] = rb[j];
        }
        __syncthreads();
        if (k0 + kStage < p.kpad) {
#pragma unroll
            for (int j = 0; j < kRows; ++j) {
                const int k = k0 + kStage + row0 + 4 * j;
                ra[j] = k < p.kpad ? wcol[(size_t)k * p.cinpad] : 0.0f;
                rb[j] = seg_gather_dy<KS>(p, k, pixel_valid, map_dy, py0, px0);
            }
        }
        if (active) {
            const int quads = min(kStage, p.kpad - k0) >> 2;
            for (int kk = 0; kk < quads; ++kk) {
                const float a = As[(kk * 4 + frow) * kPitch + wave * 16 + fcol];
#pragma unroll
                for (int n = 0; n < 4; ++n)
                    acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Bs[(kk * 4 + frow) * kPitch + n * 16 + fcol], acc[n], 0, 0, 0);
            }
            if ((step & (kSlabStages - 1)) == kSlabStages - 1) {
#pragma unroll
                for (int n = 0; n < 4; ++n) { tot[n] += acc[n]; acc[n] = f32x4{0.f, 0.f, 0.f, 0.f}; }
            }
        }
    }
    if (!active) return;
    if (step & (kSlabStages - 1)) {
#pragma unroll
        for (int n = 0; n < 4; ++n) tot[n] += acc[n];
    }
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int op = blockIdx.x * kUnetTile + n * 16 + fcol;
        if (op >= npix) continue;
        const int om = op / cells, rem = op - om * cells;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ci = ci0 + wave * 16 + 4 * frow + r;
            if (ci >= cin) continue;
            const int64_t o = ((int64_t)om * cin + ci) * cells + rem;
            float v = tot[n][r];
            if (p.residual) v += p.residual[o];
            p.out[o] = v;
        }
    }
}

// wt[k][ci] = w[co][ci][ks-1-ty][ks-1-tx] with k = co ks^2 + ty ks + tx (zero beyond k and cin); zero_bias[ci] = 0
__global__ __launch_bounds__(256) void segtrain_flip_kernel(const float *w, float *wt, float *zero_bias, int cout, int cin, int ks, int kpad, int cinpad)
{
    const int64_t n = (int64_t)kpad * cinpad, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const int k = (int)(i / cinpad), ci = (int)(i - (int64_t)k * cinpad), taps = ks * ks;
        const int co = k / taps, tap = k - co * taps;
        wt[i] = (co < cout && ci < cin) ? w[((int64_t)co * cin + ci) * taps + (taps - 1 - tap)] : 0.0f;
    } else if (i < n + cinpad) {
        zero_bias[i - n] = 0.0f;
    }
}

// The gradient of the virtual input up2x(a) ++ skip: da = the 2 x 2 sum of the first ca channels in the order (0,0) (0,1) (1,0)
// (1,1) (a copy without upsample); the rest goes to, or is added into, the skip's gradient.
__global__ __launch_bounds__(256) void segtrain_split_kernel(const float *dcat, float *da, float *dskip, int num_maps, int ca, int cb, int h, int w,
                                                             int upsample, int accumulate)
{
    const int ha = upsample ? h >> 1 : h, wa = upsample ? w >> 1 : w;
    const int64_t na = (int64_t)num_maps * ca * ha * wa, nb = (int64_t)num_maps * cb * h * w, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < na) {
        if (!da) return;
        const int x = (int)(i % wa), y = (int)((i / wa) % ha), c = (int)((i / ((int64_t)wa * ha)) % ca), m = (int)(i / ((int64_t)wa * ha * ca));
        const float *src = dcat + ((int64_t)m * (ca + cb) + c) * h * w;
        float v;
        if (upsample) {
            const float *q = src + (int64_t)(2 * y) * w + 2 * x;
            v = ((q[0] + q[1]) + q[w]) + q[w + 1];
        } else {
            v = src[(int64_t)y * w + x];
        }
        da[i] = accumulate ? da[i] + v : v;
    } else if (i < na + nb) {
        if (!dskip) return;
        const int64_t j = i - na, plane = (int64_t)h * w;
        const int m = (int)(j / (plane * cb));
        const int64_t rest = j - (int64_t)m * plane * cb;
        const float v = dcat[((int64_t)m * (ca + cb) + ca) * plane + rest];
        dskip[j] = accumulate ? dskip[j] + v : v;
    }
}

// ---- float64 reductions ----
__device__ __forceinline__ double seg_block_sum(double v, double *red)
{
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

__device__ __forceinline__ int64_t seg_channel_index(int i, int c, int channels, int cells)
{
    const int m = i / cells;
    return ((int64_t)m * channels + c) * cells + (i - m * cells);
}

__global__ __launch_bounds__(256) void segtrain_bias_grad_kernel(const float *dy, float *db, int num_maps, int channels, int cells)
{
    __shared__ double red[256];
    const int c = blockIdx.x, n = num_maps * cells;
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += (double)dy[seg_channel_index(i, c, channels, cells)];
    s = seg_block_sum(s, red);
    if (threadIdx.x == 0) db[c] = (float)s;
}

// stats[c] = mean, stats[channels + c] = 1 / sqrt(biased variance + eps); the running statistics take the unbiased variance
__global__ __launch_bounds__(256) void segtrain_bn_stats_kernel(const float *x, double *stats, float *running_mean, float *running_var, int num_maps,
                                                                int channels, int cells)
{
    __shared__ double red[256];
    const int c = blockIdx.x, n = num_maps * cells;
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += (double)x[seg_channel_index(i, c, channels, cells)];
    const double mean = seg_block_sum(s, red) / n;
    s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const double d = (double)x[seg_channel_index(i, c, channels, cells)] - mean;
        s += d * d;
    }
    const double ss = seg_block_sum(s, red);
    if (threadIdx.x) return;
    stats[c] = mean;
    stats[channels + c] = 1.0 / sqrt(ss / n + kSegBnEps);
    if (running_mean) running_mean[c] = (float)((1.0 - kSegBnMomentum) * (double)running_mean[c] + kSegBnMomentum * mean);
    if (running_var) running_var[c] = (float)((1.0 - kSegBnMomentum) * (double)running_var[c] + kSegBnMomentum * (ss / (n - 1)));
}

__global__ __launch_bounds__(256) void segtrain_bn_apply_kernel(const float *x, const double *stats, const float *gamma, const float *beta,
                                                                const float *residual, int relu, float *y, int channels, int cells, int64_t total)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)((i / cells) % channels);
    double v = ((double)x[i] - stats[c]) * stats[channels + c] * (double)gamma[c] + (double)beta[c];
    if (residual) v += (double)residual[i];
    if (relu && !(v > 0.0)) v = 0.0;
    y[i] = (float)v;
}

// sums[c] = sum g, sums[channels + c] = sum g xhat with g = dy where the ReLU let the output through
__global__ __launch_bounds__(256) void segtrain_bn_bwd_sums_kernel(const float *dy, const float *y, const float *x, const double *stats, int relu,
                                                                   double *sums, float *dgamma, float *dbeta, int num_maps, int channels, int cells)
{
    __shared__ double red[256];
    const int c = blockIdx.x, n = num_maps * cells;
    const double mean = stats[c], invstd = stats[channels + c];
    double s = 0.0, sx = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int64_t o = seg_channel_index(i, c, channels, cells);
        const double g = (relu && !(y[o] > 0.0f)) ? 0.0 : (double)dy[o];
        s += g;
        sx += g * (((double)x[o] - mean) * invstd);
    }
    s = seg_block_sum(s, red);
    sx = seg_block_sum(sx, red);
    if (threadIdx.x) return;
    sums[c] = s;
    sums[channels + c] = sx;
    dbeta[c] = (float)s;
    dgamma[c] = (float)sx;
}

// dx may be dy's own buffer (each element is read, then written, by one thread); dres receives the masked gradient
__global__ __launch_bounds__(256) void segtrain_bn_bwd_dx_kernel(const float *dy, const float *y, const float *x, const double *stats, const double *sums,
                                                                 const float *gamma, int relu, float *dx, float *dres, int channels, int cells,
                                                                 double inv_n, int64_t total)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)((i / cells) % channels);
    const float g32 = (relu && !(y[i] > 0.0f)) ? 0.0f : dy[i];
    const double invstd = stats[channels + c], xhat = ((double)x[i] - stats[c]) * invstd;
    if (dres) dres[i] = g32;
    dx[i] = (float)((double)gamma[c] * invstd * ((double)g32 - sums[c] * inv_n - xhat * (sums[channels + c] * inv_n)));
}

// A cell receives a window's gradient iff it is the window's first maximum in row-major order (torch: val > maxval).  Up to four
// windows hold a cell; they are added in ascending (oy, ox).
__global__ __launch_bounds__(256) void segtrain_maxpool_bwd_kernel(const float *x, const float *gout, float *gin, int64_t planes, int hin, int win,
                                                                   int hout, int wout, int accumulate)
{
    const int64_t cells = (int64_t)hin * win, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= planes * cells) return;
    const int64_t pl = i / cells;
    const int rem = (int)(i - pl * cells), iy = rem / win, ix = rem - iy * win;
    const float *src = x + pl * cells, *g = gout + pl * (int64_t)hout * wout;
    float sum = 0.0f;
    for (int oy = iy >> 1; oy <= (iy + 1) >> 1; ++oy) {
        if (oy >= hout) continue;
        for (int ox = ix >> 1; ox <= (ix + 1) >> 1; ++ox) {
            if (ox >= wout) continue;
            float best = -INFINITY;
            int arg = -1;
            for (int dy = 0; dy < 3; ++dy) {
                const int yy = 2 * oy - 1 + dy;
                if (yy < 0 || yy >= hin) continue;
                for (int dx = 0; dx < 3; ++dx) {
                    const int xx = 2 * ox - 1 + dx;
                    if (xx < 0 || xx >= win) continue;
                    const float v = src[(int64_t)yy * win + xx];
                    if (v > best || arg < 0) { best = v; arg = yy * win + xx; }
                }
            }
            if (arg == rem) sum += g[(int64_t)oy * wout + ox];
        }
    }
    gin[i] = accumulate ? gin[i] + sum : sum;
}

// per cell: terms[i] = -log softmax(logits)[target] and dlogits = (softmax - onehot) / n, in float64
__global__ __launch_bounds__(256) void segtrain_ce_kernel(const float *logits, const int64_t *targets, float *dlogits, double *terms, int num_maps, int nc,
                                                          int64_t cells)
{
    const int64_t n = cells * num_maps, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t map = i / cells, cell = i - map * cells;
    const float *l = logits + map * nc * cells + cell;
    float best = l[0];
    for (int c = 1; c < nc; ++c) best = fmaxf(best, l[c * cells]);
    double sum = 0.0;
    for (int c = 0; c < nc; ++c) sum += exp((double)l[c * cells] - (double)best);
    const int64_t tg = targets[i];
    const bool ok = tg >= 0 && tg < nc;      // the wrappers reject other targets before the launch; never read out of bounds
    terms[i] = ok ? log(sum) - ((double)l[tg * cells] - (double)best) : 0.0;
    if (!dlogits) return;
    float *d = dlogits + map * nc * cells + cell;
    for (int c = 0; c < nc; ++c) d[c * cells] = (float)((exp((double)l[c * cells] - (double)best) / sum - (c == tg ? 1.0 : 0.0)) / (double)n);
}

__global__ __launch_bounds__(256) void segtrain_mean_kernel(const double *terms, float *out, int64_t n)
{
    __shared__ double red[256];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) s += terms[i];
    s = seg_block_sum(s, red);
    if (threadIdx.x == 0) out[0] = (float)(s / (double)n);
}

// torch.optim.Adam's update (weight decay added to the gradient), float64 from the float32 state, each of p, m, v rounded once
__global__ __launch_bounds__(256) void segtrain_adam_kernel(float *p, const float *g, float *m, float *v, int64_t n, double lr, double beta1, double beta2,
                                                            double eps, double weight_decay, double correction1, double correction2_sqrt)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double pi = (double)p[i], gi = (double)g[i] + weight_decay * pi;
    const double mi = beta1 * (double)m[i] + (1.0 - beta1) * gi, vi = beta2 * (double)v[i] + (1.0 - beta2) * gi * gi;
    m[i] = (float)mi;
    v[i] = (float)vi;
    p[i] = (float)(pi - (lr / correction1) * mi / (sqrt(vi) / correction2_sqrt + eps));
}

unsigned seg_blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

hipError_t seg_launch_wgrad(hipStream_t s, int ksize, const SegConvGrad &g)
{
    const dim3 grid((unsigned)((g.k + kUnetTile - 1) / kUnetTile), (unsigned)((g.cout + kUnetTile - 1) / kUnetTile), (unsigned)g.chunks);
    if (ksize == 1) segtrain_wgrad_kernel<1><<<grid, 256, 0, s>>>(g);
    else if (ksize == 3) segtrain_wgrad_kernel<3><<<grid, 256, 0, s>>>(g);
    else if (ksize == 7) segtrain_wgrad_kernel<7><<<grid, 256, 0, s>>>(g);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t seg_launch_wgrad_reduce(hipStream_t s, const float *partial, float *dw, int64_t n, int chunks)
{
    segtrain_wgrad_reduce_kernel<<<seg_blocks(n), 256, 0, s>>>(partial, dw, n, chunks);
    return hipGetLastError();
}

hipError_t seg_launch_dgrad_strided(hipStream_t s, int ksize, const SegConvGrad &g)
{
    const int64_t npix = (int64_t)g.num_maps * g.hin * g.win;
    const dim3 grid((unsigned)((npix + kUnetTile - 1) / kUnetTile), (unsigned)(g.cinpad / kUnetTile));
    if (ksize == 1) segtrain_dgrad_kernel<1><<<grid, 256, 0, s>>>(g);
    else if (ksize == 3) segtrain_dgrad_kernel<3><<<grid, 256, 0, s>>>(g);
    else if (ksize == 7) segtrain_dgrad_kernel<7><<<grid, 256, 0, s>>>(g);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t seg_launch_flip(hipStream_t s, const float *w, float *wt, float *zero_bias, int cout, int cin, int ksize, int kpad, int cinpad)
{
    segtrain_flip_kernel<<<seg_blocks((int64_t)kpad * cinpad + cinpad), 256, 0, s>>>(w, wt, zero_bias, cout, cin, ksize, kpad, cinpad);
    return hipGetLastError();
}

hipError_t seg_launch_split(hipStream_t s, const float *dcat, float *da, float *dskip, int num_maps, int ca, int cb, int h, int w, int upsample,
                            int accumulate)
{
    const int64_t na = (int64_t)num_maps * ca * (upsample ? (h >> 1) * (w >> 1) : h * w), nb = (int64_t)num_maps * cb * h * w;
    segtrain_split_kernel<<<seg_blocks(na + nb), 256, 0, s>>>(dcat, da, dskip, num_maps, ca, cb, h, w, upsample, accumulate);
    return hipGetLastError();
}

hipError_t seg_launch_bias_grad(hipStream_t s, const float *dy, float *db, int num_maps, int channels, int64_t cells)
{
    segtrain_bias_grad_kernel<<<(unsigned)channels, 256, 0, s>>>(dy, db, num_maps, channels, (int)cells);
    return hipGetLastError();
}

hipError_t seg_launch_bn_forward(hipStream_t s, const float *x, const float *gamma, const float *beta, const float *residual, int relu,
                                 float *running_mean, float *running_var, float *y, double *stats, int num_maps, int channels, int64_t cells)
{
    segtrain_bn_stats_kernel<<<(unsigned)channels, 256, 0, s>>>(x, stats, running_mean, running_var, num_maps, channels, (int)cells);
    if (hipError_t e = hipGetLastError()) return e;
    const int64_t total = (int64_t)num_maps * channels * cells;
    segtrain_bn_apply_kernel<<<seg_blocks(total), 256, 0, s>>>(x, stats, gamma, beta, residual, relu, y, channels, (int)cells, total);
    return hipGetLastError();
}

hipError_t seg_launch_bn_backward(hipStream_t s, const float *dy, const float *y, const float *x, const double *stats, const float *gamma, int relu,
                                  float *dx, float *dres, float *dgamma, float *dbeta, double *sums, int num_maps, int channels, int64_t cells)
{
    segtrain_bn_bwd_sums_kernel<<<(unsigned)channels, 256, 0, s>>>(dy, y, x, stats, relu, sums, dgamma, dbeta, num_maps, channels, (int)cells);
    if (hipError_t e = hipGetLastError()) return e;
    const int64_t total = (int64_t)num_maps * channels * cells;
    segtrain_bn_bwd_dx_kernel<<<seg_blocks(total), 256, 0, s>>>(dy, y, x, stats, sums, gamma, relu, dx, dres, channels, (int)cells,
                                                                1.0 / (double)(num_maps * cells), total);
    return hipGetLastError();
}

hipError_t seg_launch_maxpool_backward(hipStream_t s, const float *x, const float *gout, float *gin, int64_t planes, int hin, int win, int accumulate)
{
    segtrain_maxpool_bwd_kernel<<<seg_blocks(planes * hin * win), 256, 0, s>>>(x, gout, gin, planes, hin, win, (hin - 1) / 2 + 1, (win - 1) / 2 + 1,
                                                                              accumulate);
    return hipGetLastError();
}

hipError_t seg_launch_cross_entropy(hipStream_t s, const float *logits, const int64_t *targets, float *dlogits, double *terms, float *loss,
                                    int num_maps, int classes, int64_t cells)
{
    const int64_t n = cells * num_maps;
    segtrain_ce_kernel<<<seg_blocks(n), 256, 0, s>>>(logits, targets, dlogits, terms, num_maps, classes, cells);
    if (hipError_t e = hipGetLastError()) return e;
    segtrain_mean_kernel<<<1, 256, 0, s>>>(terms, loss, n);
    return hipGetLastError();
}

hipError_t seg_launch_adam(hipStream_t s, float *p, const float *g, float *m, float *v, int64_t n, double lr, double beta1, double beta2, double eps,
                           double weight_decay, double correction1, double correction2_sqrt)
{
    segtrain_adam_kernel<<<seg_blocks(n), 256, 0, s>>>(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, correction1, correction2_sqrt);
    return hipGetLastError();
}

}  // namespace bn
