// unet_kernels.hip -- the U-Net terrain classifier's kernels: one fused convolution family on the exact float32
// MFMA, the max-pool, the head's softmax / argmax and the weight re-layout.  Host side: unet_host.cpp, shared types: unet_handle.h;
// the staging constants and the gather, shared with the training kernels: unet_conv_tile.h.
//
// The convolution is an implicit GEMM  out[co][pixel] = sum_k wt[k][co] * x[k][pixel]  with k = ci * ksize^2 + ky * ksize + kx
// (the order of a PyTorch weight row) and pixel = (map, oy, ox).  A workgroup of four waves owns 64 output channels x 64 pixels;
// wave w owns channels 16 w ... 16 w + 15 as four 16 x 16 accumulators of v_mfma_f32_16x16x4_f32.  Per step 64 k rows of both
// operands go through LDS (row pitch 80 floats: the four k rows a fragment read touches fall on disjoint banks), the next step's
// rows are already in flight in registers (32 loads per lane).  The deep layers have few pixels and walk their K serially on a
// handful of workgroups: DESIGN.md 4.11 has the measured cost of that and what would change it.
//
// Summation order (what makes the bits a function of the weights and the map's own pixels alone): an output element is the sum over
// slabs of 128 consecutive k of one k-ordered fmaf chain each (the MFMA's own order), the slab sums added in ascending order.  The
// partition depends on k only -- not on the tile, the batch or the launch -- there is no split over workgroups and no atomic.
#include "unet_conv_tile.h"
#include "unet_handle.h"

namespace bn {
namespace {

template <int KS>
__global__ __launch_bounds__(256) void unet_conv_kernel(const UnetConvArgs p)
{
    __shared__ float As[kStage * kPitch], Bs[kStage * kPitch];
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);      // the wave index, as a scalar
    const int col = lane, row0 = wave;                   // staging role: column col of k rows row0, row0 + 4, ... of the stage
    const int64_t cells = (int64_t)p.hout * p.wout, npix = cells * p.num_maps;
    const int64_t pix = (int64_t)blockIdx.x * kUnetTile + col;
    const bool pixel_valid = pix < npix;
    int map = 0, iy0 = 0, ix0 = 0;
    if (pixel_valid) {
        map = (int)(pix / cells);
        const int rem = (int)(pix - (int64_t)map * cells), oy = rem / p.wout;
        iy0 = oy * p.stride - p.pad;
        ix0 = (rem - oy * p.wout) * p.stride - p.pad;
    }
    const int plane_a = p.upsample ? (p.hin >> 1) * (p.win >> 1) : p.hin * p.win;
    const float *map_a = p.a + (int64_t)map * p.ca * plane_a, *map_b = p.b + (int64_t)map * p.cb * (p.hin * p.win);
    const int co0 = blockIdx.y * kUnetTile;
    const float *wcol = p.wt + co0 + col;
    const bool active = co0 + wave * 16 < p.cout;        // a wave whose 16 channels are all padding only stages

    float ra[kRows], rb[kRows];
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
        const int k = row0 + 4 * j;
        ra[j] = k < p.kpad ? wcol[(size_t)k * p.coutpad] : 0.0f;
        rb[j] = unet_gather<KS>(p, k, pixel_valid, map_a, map_b, iy0, ix0);
    }
    f32x4 acc[4], tot[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) { acc[n] = f32x4{0.f, 0.f, 0.f, 0.f}; tot[n] = f32x4{0.f, 0.f, 0.f, 0.f}; }

    const int frow = lane >> 4, fcol = lane & 15;
    int step = 0;
    for (int k0 = 0; k0 < p.kpad; k0 += kStage, ++step) {
        __syncthreads();                                 // the previous stage's fragment reads are done
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
                ra[j] = k < p.kpad ? wcol[(size_t)k * p.coutpad] : 0.0f;
                rb[j] = unet_gather<KS>(p, k, pixel_valid, map_a, map_b, iy0, ix0);
            }
        }
        if (active) {
            auto quad = [&](int kk) {                    // four k rows: one MFMA step of each accumulator
                const float a = As[(kk * 4 + frow) * kPitch + wave * 16 + fcol];
#pragma unroll
                for (int n = 0; n < 4; ++n)
                    acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Bs[(kk * 4 + frow) * kPitch + n * 16 + fcol], acc[n], 0, 0, 0);
            };
            const int quads = min(kStage, p.kpad - k0) >> 2;    // the last stage may be short: kpad is a multiple of 16 only
            if (quads == kStage / 4) {
#pragma unroll
                for (int kk = 0; kk < kStage / 4; ++kk) quad(kk);
            } else {
                for (int kk = 0; kk < quads; ++kk) quad(kk);
            }
            if ((step & (kSlabStages - 1)) == kSlabStages - 1) {
#pragma unroll
                for (int n = 0; n < 4; ++n) { tot[n] += acc[n]; acc[n] = f32x4{0.f, 0.f, 0.f, 0.f}; }
            }
        }
    }
    if (!active) return;
    if (step & (kSlabStages - 1)) {                      // the last slab holds one stage only
#pragma unroll
        for (int n = 0; n < 4; ++n) tot[n] += acc[n];
    }
    // C/D map of the 16 x 16 MFMA: column (pixel) = lane & 15, row (channel) = 4 (lane >> 4) + register
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int64_t op = (int64_t)blockIdx.x * kUnetTile + n * 16 + fcol;
        if (op >= npix) continue;
        const int64_t om = op / cells, rem = op - om * cells;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int co = co0 + wave * 16 + 4 * frow + r;
            if (co >= p.cout) continue;
            const int64_t o = (om * p.cout + co) * cells + rem;
            float v = tot[n][r] + p.bias[co];
            if (p.residual) v += p.residual[o];
            if (p.relu) v = fmaxf(v, 0.0f);
            p.out[o] = v;
        }
    }
}

// wt[k][co] = w[co][k] (zero beyond k and cout), bias_pad[co] = bias[co] (zero beyond cout, or everywhere without a bias)
__global__ __launch_bounds__(256) void unet_relayout_kernel(const float *w, const float *bias, float *wt, float *bias_pad, int cout, int k,
                                                            int kpad, int coutpad)
{
    const int64_t n = (int64_t)kpad * coutpad, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const int kk = (int)(i / coutpad), co = (int)(i - (int64_t)kk * coutpad);
        wt[i] = (kk < k && co < cout) ? w[(int64_t)co * k + kk] : 0.0f;
    } else if (i < n + coutpad) {
        const int co = (int)(i - n);
        bias_pad[co] = (bias && co < cout) ? bias[co] : 0.0f;
    }
}

// 3 x 3, stride 2, pad 1; padding counts as -inf (a window always holds at least one real cell)
__global__ __launch_bounds__(256) void unet_maxpool_kernel(const float *in, float *out, int64_t planes, int hin, int win, int hout, int wout)
{
    const int64_t cells = (int64_t)hout * wout, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= planes * cells) return;
    const int64_t pl = i / cells;
    const int rem = (int)(i - pl * cells), oy = rem / wout, ox = rem - oy * wout;
    const float *src = in + pl * (int64_t)hin * win;
    float m = -INFINITY;
    for (int dy = 0; dy < 3; ++dy) {
        const int iy = 2 * oy - 1 + dy;
        if (iy < 0 || iy >= hin) continue;
        for (int dx = 0; dx < 3; ++dx) {
            const int ix = 2 * ox - 1 + dx;
            if (ix < 0 || ix >= win) continue;
            m = fmaxf(m, src[(int64_t)iy * win + ix]);
        }
    }
    out[i] = m;
}

// per cell: the class map is the argmax of the logits (the lowest index wins a tie); the probabilities are the softmax evaluated
// in float64 and rounded once
__global__ __launch_bounds__(256) void unet_head_kernel(const float *logits, float *prob, int32_t *cls, int num_maps, int nc, int64_t cells)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= cells * num_maps) return;
    const int64_t map = i / cells, cell = i - map * cells;
    const float *l = logits + map * nc * cells + cell;
    float best = l[0];
    int arg = 0;
    for (int c = 1; c < nc; ++c) {
        const float v = l[c * cells];
        if (v > best) { best = v; arg = c; }
    }
    if (cls) cls[i] = arg;
    if (!prob) return;
    double sum = 0.0;
    for (int c = 0; c < nc; ++c) sum += exp((double)l[c * cells] - (double)best);
    float *q = prob + map * nc * cells + cell;
    for (int c = 0; c < nc; ++c) q[c * cells] = (float)(exp((double)l[c * cells] - (double)best) / sum);
}

}  // namespace

hipError_t unet_launch_conv(hipStream_t stream, int ksize, const UnetConvArgs &a)
{
    const int64_t npix = (int64_t)a.num_maps * a.hout * a.wout;
    const dim3 grid((unsigned)((npix + kUnetTile - 1) / kUnetTile), (unsigned)(a.coutpad / kUnetTile));
    if (ksize == 1) unet_conv_kernel<1><<<grid, 256, 0, stream>>>(a);
    else if (ksize == 3) unet_conv_kernel<3><<<grid, 256, 0, stream>>>(a);
    else if (ksize == 7) unet_conv_kernel<7><<<grid, 256, 0, stream>>>(a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t unet_launch_relayout(hipStream_t stream, const float *w, const float *bias, float *wt, float *bias_pad, int cout, int k, int kpad, int coutpad)
{
    const int64_t n = (int64_t)kpad * coutpad + coutpad;
    unet_relayout_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(w, bias, wt, bias_pad, cout, k, kpad, coutpad);
    return hipGetLastError();
}

hipError_t unet_launch_maxpool(hipStream_t stream, const float *in, float *out, int64_t planes, int hin, int win, int hout, int wout)
{
    const int64_t n = planes * hout * wout;
    unet_maxpool_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(in, out, planes, hin, win, hout, wout);
    return hipGetLastError();
}

hipError_t unet_launch_head(hipStream_t stream, const float *logits, float *probabilities, int32_t *classes, int num_maps, int num_classes, int64_t cells)
{
    const int64_t n = cells * num_maps;
    unet_head_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(logits, probabilities, classes, num_maps, num_classes, cells);
    return hipGetLastError();
}

}  // namespace bn
