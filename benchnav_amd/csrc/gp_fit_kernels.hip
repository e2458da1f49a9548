// gp_fit_kernels.hip -- fitting the exact-GP slip regressors on the device: RegressorTrainer.train's Adam on the
// exact marginal log-likelihood of ExactGP(ConstantMean, ScaleKernel(RBFKernel), GaussianLikelihood) on a 1-D input
// (src/prediction_models/trainers/regressor_trainer.py:128-170), from the model's equations in float64.
//
//   theta = (constant, raw_outputscale, raw_lengthscale, raw_noise);  c = constant, s = softplus(raw_outputscale),
//   l = softplus(raw_lengthscale), noise = softplus(raw_noise) + lower_bound
//   K = s exp(-(x - x')^2 / (2 l^2)) + noise I = L L^T,  r = y - c,  z = L^-1 r,  alpha = L^-T z
//   loss = [ |z|^2 + 2 sum log L_ii + N log 2 pi ] / (2 N)
//   dloss/dc = -sum alpha / N,  dloss/dpsi = tr((K^-1 - alpha alpha^T) dK/dpsi) / (2 N),  psi in {s, l, noise}
//
// The matrices are row-major with the order padded to the panel width 32 (identity on the padding's diagonal), and only the
// 32 x 32 tiles on and below the diagonal exist.  One evaluation is this chain of launches on the caller's stream:
//   gp_fit_build_kernel     K's tiles from x and the device-resident hyperparameters
//   per panel p:            gp_fit_potrf_kernel   one wave factorises the diagonal tile in registers and leaves its explicit inverse
//                           gp_fit_trsm_kernel    the tiles below it times that inverse transposed (MFMA)
//                           gp_fit_syrk_kernel    the rank-32 update of the trailing tiles (MFMA)
//   gp_fit_inverse_kernel   X = L^-1, one workgroup per block column: X[i,j] = -L_ii^-1 sum_k L[i,k] X[k,j] (MFMA)
//   gp_fit_z_kernel, gp_fit_alpha_kernel          z = X r, alpha = X^T z
//   gp_fit_grad_kernel      the tiles of K^-1 = X^T X in MFMA accumulators (never stored), weighted by (K^-1 - alpha alpha^T) and
//                           the three dK/dpsi regenerated from x, reduced to three partial sums per tile
//   gp_fit_loss_kernel      every remaining sum in an order fixed by N alone; loss and the raw gradient
//   gp_fit_adam_kernel      one thread: the history entry, torch.optim.Adam's update, the next hyperparameters
// No floating-point atomics: two fits of the same data give the same bits.  A pivot that is not positive and finite sets the
// status word and the iteration number; every later kernel returns at once when it sees the word.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "bn_host.h"
#include "gp_handle.h"

namespace bn {
namespace {

constexpr int kFitMaxPoints = 10240;     // bn_gp_max_points()
constexpr int kFitNB = 32;               // panel width and tile order
constexpr int kFitTile = kFitNB * kFitNB;
constexpr int kFitHistory = 16384;       // iterations a handle can record
constexpr int kFitInvWaves = 16;         // gp_fit_inverse_kernel: four k groups of four waves (one 16 x 16 quadrant each)
constexpr double kLog2Pi = 1.8378770664093454835606594728112;

using f64x4 = __attribute__((ext_vector_type(4))) double;

struct GpFitState {
    double raw[4], m[4], v[4];           // theta and Adam's moments
    double hyp[5];                       // c, s, l, noise, 2 l^2
    double lower_bound;
    double loss, grad[4];                // of the last evaluation, the gradient with respect to theta
    int32_t status, failed_iteration, iteration, adam_step;
};

struct GpFitDev {
    GpFitState *st;
    const double *x, *y;                 // (npad), zero beyond n
    double *A, *X;                       // (npad, npad): K then L; L^-1
    double *dinv;                        // (T, 32, 32): the inverses of L's diagonal tiles
    double *z, *alpha;                   // (npad)
    double *part;                        // (T (T + 1) / 2, 3)
    int32_t n, npad, T;
};

__device__ __forceinline__ f64x4 fit_mfma(double a, double b, f64x4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// the same butterfly in every wave: all lanes end with the sum
__device__ __forceinline__ double fit_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__host__ __device__ inline double fit_softplus(double v) { return v > 0.0 ? v + log1p(exp(-v)) : log1p(exp(v)); }

__global__ __launch_bounds__(256) void gp_fit_build_kernel(GpFitDev a)
{
    if (a.st->status) return;
    const int I = blockIdx.y, J = blockIdx.x, t = threadIdx.x;
    if (J > I) return;
    const double s = a.st->hyp[1], noise = a.st->hyp[3], den = a.st->hyp[4];
    for (int e = t; e < kFitTile; e += 256) {
        const int i = kFitNB * I + (e >> 5), j = kFitNB * J + (e & 31);
        double v;
        if (i < a.n && j < a.n) {
            const double d = a.x[i] - a.x[j];
            v = s * exp(-(d * d) / den);         // the specification's own operations: only exp's rounding differs from it
            if (i == j) v += noise;
        } else {
            v = i == j ? 1.0 : 0.0;
        }
        a.A[(size_t)i * a.npad + j] = v;
    }
}

// One wave: the diagonal tile p, right-looking; lane t holds row t in registers (lanes 32-63 mirror lanes 0-31 and store nothing)
// and takes the pivot and the column entries of the other rows by wave shuffles: no barrier and no LDS traffic in the factorisation.
// Leaves L_pp in A and L_pp^-1 (upper part zero; column t by forward substitution in lane t, L read from LDS) in dinv.
__global__ __launch_bounds__(64) void gp_fit_potrf_kernel(GpFitDev a, int p)
{
    __shared__ double L[kFitNB][kFitNB + 1];
    if (a.st->status) return;
    const int t = threadIdx.x, tr = t & (kFitNB - 1);
    double *blk = a.A + (size_t)kFitNB * p * a.npad + kFitNB * p;
    double row[kFitNB];
#pragma unroll
    for (int j = 0; j < kFitNB; ++j) row[j] = blk[(size_t)tr * a.npad + j];
#pragma unroll
    for (int k = 0; k < kFitNB; ++k) {
        const double piv = __shfl(row[k], k);
        if (!(piv > 0.0) || !(piv < INFINITY)) {         // the same value in every lane
            if (t == 0) { a.st->failed_iteration = a.st->iteration; a.st->status = 1; }
            return;
        }
        const double d = sqrt(piv);
        row[k] = tr == k ? d : row[k] / d;               // the rows above k hold nothing of L in column k and are not read below
#pragma unroll
        for (int j = k + 1; j < kFitNB; ++j) {
            const double ljk = __shfl(row[k], j);
            if (j <= tr) row[j] = __builtin_fma(-row[k], ljk, row[j]);
        }
    }
    if (t < kFitNB) {
#pragma unroll
        for (int j = 0; j < kFitNB; ++j) {
            L[t][j] = row[j];
            if (j <= t) blk[(size_t)t * a.npad + j] = row[j];
        }
    }
    __syncthreads();
    double v[kFitNB];                                    // column tr of the inverse
#pragma unroll
    for (int i = 0; i < kFitNB; ++i) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < i; ++k) s = k >= tr ? __builtin_fma(L[i][k], v[k], s) : s;
        v[i] = i < tr ? 0.0 : (i == tr ? 1.0 / L[i][i] : -s / L[i][i]);
    }
    if (t < kFitNB) {
        double *dv = a.dinv + (size_t)kFitTile * p + t;
#pragma unroll
        for (int i = 0; i < kFitNB; ++i) dv[i * kFitNB] = v[i];
    }
}

// L[i,p] = A[i,p] L_pp^-T for the rows below the diagonal tile: wave w of the grid takes 16 rows, all of them read before any is written.
__global__ __launch_bounds__(256) void gp_fit_trsm_kernel(GpFitDev a, int p)
{
    if (a.st->status) return;
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int r0 = kFitNB * (p + 1) + 16 * (blockIdx.x * 4 + w);
    if (r0 >= a.npad) return;
    double *row = a.A + (size_t)(r0 + (l & 15)) * a.npad + kFitNB * p + (l >> 4);
    const double *dv = a.dinv + (size_t)kFitTile * p + (l & 15) * kFitNB + (l >> 4);
    double av[8];
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) av[kk] = row[4 * kk];
    f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
        acc0 = fit_mfma(av[kk], dv[4 * kk], acc0);
        acc1 = fit_mfma(av[kk], dv[16 * kFitNB + 4 * kk], acc1);
    }
    double *out = a.A + (size_t)(r0 + (l >> 4)) * a.npad + kFitNB * p + (l & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        out[(size_t)4 * r * a.npad] = acc0[r];
        out[(size_t)4 * r * a.npad + 16] = acc1[r];
    }
}

// A[I,J] -= L[I,p] L[J,p]^T for p < J <= I: one wave per 32 x 32 tile, four accumulators.
__global__ __launch_bounds__(256) void gp_fit_syrk_kernel(GpFitDev a, int p)
{
    if (a.st->status) return;
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int I = p + 1 + blockIdx.y, J = p + 1 + blockIdx.x * 4 + w;
    if (I >= a.T || J > I) return;
    const double *li = a.A + (size_t)(kFitNB * I + (l & 15)) * a.npad + kFitNB * p + (l >> 4);
    const double *lj = a.A + (size_t)(kFitNB * J + (l & 15)) * a.npad + kFitNB * p + (l >> 4);
    const size_t half = (size_t)16 * a.npad;
    f64x4 acc[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) acc[u][v] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
        const double a0 = li[4 * kk], a1 = li[half + 4 * kk], b0 = lj[4 * kk], b1 = lj[half + 4 * kk];
        acc[0][0] = fit_mfma(a0, b0, acc[0][0]);
        acc[0][1] = fit_mfma(a0, b1, acc[0][1]);
        acc[1][0] = fit_mfma(a1, b0, acc[1][0]);
        acc[1][1] = fit_mfma(a1, b1, acc[1][1]);
    }
    double *c = a.A + (size_t)(kFitNB * I + (l >> 4)) * a.npad + kFitNB * J + (l & 15);
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double *e = c + (size_t)(16 * u + 4 * r) * a.npad + 16 * v;
                *e = *e - acc[u][v][r];
            }
}

// X = L^-1, block column j per workgroup, block row after block row.  Wave (g, qd): k group g takes the k tiles j + g, j + g + 4,
// ... in ascending order for the 16 x 16 quadrant qd of S = sum_k L[i,k] X[k,j]; the four groups' partial S go through LDS and are
// added in the order ((0 + 1) + 2) + 3 by the waves of group 0, which multiply by -L_ii^-1 and store X[i,j].  The workgroup reads
// back from global memory only what it has stored itself, a barrier earlier.
__global__ __launch_bounds__(kFitInvWaves * 64) void gp_fit_inverse_kernel(GpFitDev a)
{
    __shared__ double S[4][kFitNB][kFitNB];
    if (a.st->status) return;
    const int j = blockIdx.x, t = threadIdx.x;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6), l = t & 63, g = w >> 2, qr = (w >> 1) & 1, qc = w & 1;
    const size_t ld = a.npad;
    {
        const double *dv = a.dinv + (size_t)kFitTile * j;
        const int r = t >> 5, c = t & 31;
        a.X[(size_t)(kFitNB * j + r) * ld + kFitNB * j + c] = dv[t];
    }
    __threadfence_block();
    __syncthreads();
    for (int i = j + 1; i < a.T; ++i) {
        f64x4 acc = {0.0, 0.0, 0.0, 0.0};
        const double *lrow = a.A + (size_t)(kFitNB * i + 16 * qr + (l & 15)) * ld + (l >> 4);
        const double *xcol = a.X + (size_t)(l >> 4) * ld + kFitNB * j + 16 * qc + (l & 15);
        for (int k = j + g; k < i; k += 4) {
            const double *la = lrow + kFitNB * k, *xb = xcol + (size_t)kFitNB * k * ld;
            double av[8], bv[8];
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) { av[kk] = la[4 * kk]; bv[kk] = xb[(size_t)4 * kk * ld]; }
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) acc = fit_mfma(av[kk], bv[kk], acc);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) S[g][16 * qr + (l >> 4) + 4 * r][16 * qc + (l & 15)] = acc[r];
        __syncthreads();
        if (g == 0) {
            const double *dv = a.dinv + (size_t)kFitTile * i + (16 * qr + (l & 15)) * kFitNB + (l >> 4);
            f64x4 o = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) {
                const int kr = 4 * kk + (l >> 4), kc = 16 * qc + (l & 15);
                const double b = ((S[0][kr][kc] + S[1][kr][kc]) + S[2][kr][kc]) + S[3][kr][kc];
                o = fit_mfma(dv[4 * kk], b, o);
            }
            double *out = a.X + (size_t)(kFitNB * i + 16 * qr + (l >> 4)) * ld + kFitNB * j + 16 * qc + (l & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(size_t)4 * r * ld] = -o[r];
        }
        __threadfence_block();
        __syncthreads();
    }
}

// z = X (y - c): one wave per row, lane l sums the columns l, l + 64, ... in ascending order, then the butterfly
__global__ __launch_bounds__(256) void gp_fit_z_kernel(GpFitDev a)
{
    if (a.st->status) return;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
    if (i >= a.npad) return;
    const double c = a.st->hyp[0];
    double s = 0.0;
    if (i < a.n) {
        const double *row = a.X + (size_t)i * a.npad;
        for (int j = l; j <= i; j += 64) s = __builtin_fma(row[j], a.y[j] - c, s);
    }
    s = fit_wave_sum(s);
    if (l == 0) a.z[i] = s;
}

// alpha = X^T z: one workgroup per 32 columns, row group g sums the rows 32 J + g, + 8, ... in ascending order; thread c adds the eight
__global__ __launch_bounds__(256) void gp_fit_alpha_kernel(GpFitDev a)
{
    __shared__ double part[8][kFitNB];
    if (a.st->status) return;
    const int J = blockIdx.x, c = threadIdx.x & 31, g = threadIdx.x >> 5;
    const double *col = a.X + kFitNB * J + c;
    double s = 0.0;
    for (int i = kFitNB * J + g; i < a.npad; i += 8) s = __builtin_fma(col[(size_t)i * a.npad], a.z[i], s);
    part[g][c] = s;
    __syncthreads();
    if (g == 0) {
        double tot = 0.0;
        for (int k = 0; k < 8; ++k) tot += part[k][c];
        a.alpha[kFitNB * J + c] = tot;
    }
}

// One wave per tile (Ta, Tb), Tb <= Ta, of K^-1 = X^T X: the rows of X from 32 Ta down (X is zero above its diagonal).  The
// epilogue weights the 1024 elements; a tile off the diagonal stands for its mirror image too.
__global__ __launch_bounds__(256) void gp_fit_grad_kernel(GpFitDev a)
{
    if (a.st->status) return;
    const int idx = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
    if (idx >= a.T * (a.T + 1) / 2) return;
    int Ta = (int)((sqrt(8.0 * idx + 1.0) - 1.0) * 0.5);
    while ((Ta + 1) * (Ta + 2) / 2 <= idx) ++Ta;
    while (Ta * (Ta + 1) / 2 > idx) --Ta;
    const int Tb = idx - Ta * (Ta + 1) / 2;
    const size_t ld = a.npad;
    const double *xa = a.X + (size_t)(kFitNB * Ta + (l >> 4)) * ld + kFitNB * Ta + (l & 15);
    const double *xb = a.X + (size_t)(kFitNB * Ta + (l >> 4)) * ld + kFitNB * Tb + (l & 15);
    f64x4 acc[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) acc[u][v] = f64x4{0.0, 0.0, 0.0, 0.0};
    const int steps = (a.npad - kFitNB * Ta) / 4;
    for (int k = 0; k < steps; ++k) {
        const size_t o = (size_t)4 * k * ld;
        const double a0 = xa[o], a1 = xa[o + 16], b0 = xb[o], b1 = xb[o + 16];
        acc[0][0] = fit_mfma(a0, b0, acc[0][0]);
        acc[0][1] = fit_mfma(a0, b1, acc[0][1]);
        acc[1][0] = fit_mfma(a1, b0, acc[1][0]);
        acc[1][1] = fit_mfma(a1, b1, acc[1][1]);
    }
    const double den = a.st->hyp[4];
    double gs = 0.0, gl = 0.0, gn = 0.0;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ia = kFitNB * Ta + 16 * u + (l >> 4) + 4 * r, ib = kFitNB * Tb + 16 * v + (l & 15);
                if (ia < a.n && ib < a.n) {
                    const double wgt = acc[u][v][r] - a.alpha[ia] * a.alpha[ib];
                    const double d = a.x[ia] - a.x[ib], d2 = d * d, e = exp(-d2 / den);
                    gs = __builtin_fma(wgt, e, gs);
                    gl = __builtin_fma(wgt, e * d2, gl);
                    if (ia == ib) gn += wgt;
                }
            }
    gs = fit_wave_sum(gs);
    gl = fit_wave_sum(gl);
    gn = fit_wave_sum(gn);
    if (l == 0) {
        const double two = Ta == Tb ? 1.0 : 2.0;
        a.part[(size_t)3 * idx] = two * gs;
        a.part[(size_t)3 * idx + 1] = two * gl;
        a.part[(size_t)3 * idx + 2] = two * gn;
    }
}

// One workgroup: thread t sums the entries t, t + 256, ... in ascending order, then a binary tree over the 256 partials.
__global__ __launch_bounds__(256) void gp_fit_loss_kernel(GpFitDev a)
{
    __shared__ double red[256];
    if (a.st->status) return;
    const int t = threadIdx.x, n = a.n, ntile = a.T * (a.T + 1) / 2;
    auto block_sum = [&](double v) {
        red[t] = v;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (t < s) red[t] += red[t + s];
            __syncthreads();
        }
        const double r = red[0];
        __syncthreads();
        return r;
    };
    double ld = 0.0, zz = 0.0, sa = 0.0, g[3] = {0.0, 0.0, 0.0};
    for (int i = t; i < n; i += 256) {
        ld += log(a.A[(size_t)i * a.npad + i]);
        zz = __builtin_fma(a.z[i], a.z[i], zz);
        sa += a.alpha[i];
    }
    for (int k = t; k < ntile; k += 256)
        for (int c = 0; c < 3; ++c) g[c] += a.part[(size_t)3 * k + c];
    ld = block_sum(ld);
    zz = block_sum(zz);
    sa = block_sum(sa);
    for (int c = 0; c < 3; ++c) g[c] = block_sum(g[c]);
    if (t == 0) {
        GpFitState *st = a.st;
        const double s = st->hyp[1], l = st->hyp[2], dn = 2.0 * n;
        st->loss = (zz + 2.0 * ld + n * kLog2Pi) / dn;
        st->grad[0] = -sa / n;
        st->grad[1] = g[0] / dn * (1.0 / (1.0 + exp(-st->raw[1])));
        st->grad[2] = g[1] * s / (l * l * l) / dn * (1.0 / (1.0 + exp(-st->raw[2])));
        st->grad[3] = g[2] / dn * (1.0 / (1.0 + exp(-st->raw[3])));
    }
}

// torch.optim.Adam's single-tensor update (no weight decay, no amsgrad) on the four raw parameters
__global__ void gp_fit_adam_kernel(GpFitState *st, double *history, int capacity, double lr, double b1, double b2, double eps)
{
    if (threadIdx.x || blockIdx.x || st->status) return;
    const int it = st->iteration;
    if (it < capacity) history[it] = st->loss;
    const int step = ++st->adam_step;
    const double bc1 = 1.0 - pow(b1, (double)step), bc2 = 1.0 - pow(b2, (double)step);
    const double step_size = lr / bc1, bc2s = sqrt(bc2);
    for (int p = 0; p < 4; ++p) {
        const double gr = st->grad[p];
        const double m = st->m[p] + (1.0 - b1) * (gr - st->m[p]);
        const double v = st->v[p] * b2 + (1.0 - b2) * (gr * gr);
        st->m[p] = m;
        st->v[p] = v;
        const double denom = sqrt(v) / bc2s + eps;
        st->raw[p] = st->raw[p] + (-step_size) * (m / denom);
    }
    const double l = fit_softplus(st->raw[2]);
    st->hyp[0] = st->raw[0];
    st->hyp[1] = fit_softplus(st->raw[1]);
    st->hyp[2] = l;
    st->hyp[3] = fit_softplus(st->raw[3]) + st->lower_bound;
    st->hyp[4] = 2.0 * l * l;
    st->iteration = it + 1;
}

// L^-1 and into the order GpRegDev.linv is read in: row block i (16 rows), k step j < 4 (i + 1), lane
__global__ __launch_bounds__(256) void gp_fit_pack_kernel(GpFitDev a, double *linv)
{
    if (a.st->status) return;
    const int i = blockIdx.y, j = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
    if (j >= 4 * (i + 1)) return;
    const int row = 16 * i + (l & 15), col = 4 * j + (l >> 4);
    const double v = (row < a.n && col <= row) ? a.X[(size_t)row * a.npad + col] : 0.0;
    linv[(size_t)128 * i * (i + 1) + (size_t)64 * j + l] = v;
}

thread_local std::string g_fit_error;

int fit_fail(int code, const std::string &msg)
{
    g_fit_error = msg;
    return code;
}

#define FIT_HIP(expr) BN_HIP_AS(fit_fail, expr, #expr)

int fit_npad(int n) { return (n + kFitNB - 1) / kFitNB * kFitNB; }

}  // namespace
}  // namespace bn

struct bn_gp_fit {
    int device = 0, n = 0, npad = 0, T = 0;
    int enqueued = 0;                    // iterations enqueued so far
    hipStream_t last = nullptr;          // the stream of the last enqueue: bn_gp_fit_read synchronises it
    bn::DeviceBuffers bufs;
    bn::GpFitState *st = nullptr;
    double *x = nullptr, *y = nullptr, *A = nullptr, *X = nullptr, *dinv = nullptr, *z = nullptr, *alpha = nullptr, *part = nullptr,
           *history = nullptr;
    bn::GpFitDev dev() const
    {
        bn::GpFitDev d{};
        d.st = st; d.x = x; d.y = y; d.A = A; d.X = X; d.dinv = dinv; d.z = z; d.alpha = alpha; d.part = part;
        d.n = n; d.npad = npad; d.T = T;
        return d;
    }
};

namespace bn {
namespace {

// K = L L^T, X = L^-1, z and alpha at the hyperparameters in device memory; with_grad: the loss and the raw gradient too
int fit_enqueue(bn_gp_fit *h, hipStream_t s, bool with_grad)
{
    const GpFitDev d = h->dev();
    const int T = h->T;
    gp_fit_build_kernel<<<dim3(T, T), 256, 0, s>>>(d);
    for (int p = 0; p < T; ++p) {
        gp_fit_potrf_kernel<<<1, 64, 0, s>>>(d, p);
        const int below = T - p - 1;
        if (below > 0) {
            gp_fit_trsm_kernel<<<(below * 2 + 3) / 4, 256, 0, s>>>(d, p);
            gp_fit_syrk_kernel<<<dim3((below + 3) / 4, below), 256, 0, s>>>(d, p);
        }
    }
    gp_fit_inverse_kernel<<<T, kFitInvWaves * 64, 0, s>>>(d);
    gp_fit_z_kernel<<<h->npad / 4, 256, 0, s>>>(d);
    gp_fit_alpha_kernel<<<T, 256, 0, s>>>(d);
    if (with_grad) {
        gp_fit_grad_kernel<<<(T * (T + 1) / 2 + 3) / 4, 256, 0, s>>>(d);
        gp_fit_loss_kernel<<<1, 256, 0, s>>>(d);
    }
    FIT_HIP(hipGetLastError());
    h->last = s;
    return BN_OK;
}

// a fresh state at theta = raw: moments, status and iteration count cleared
int fit_state_from_raw(const double *raw, double lower_bound, GpFitState *st)
{
    *st = GpFitState{};
    st->lower_bound = lower_bound;
    const double l = fit_softplus(raw[2]);
    for (int p = 0; p < 4; ++p) st->raw[p] = raw[p];
    st->hyp[0] = raw[0]; st->hyp[1] = fit_softplus(raw[1]); st->hyp[2] = l; st->hyp[3] = fit_softplus(raw[3]) + lower_bound;
    st->hyp[4] = 2.0 * l * l;
    if (!(st->hyp[1] > 0.0) || !(l > 0.0) || !(st->hyp[3] > 0.0) || !std::isfinite(1.0 / st->hyp[4]) || 1.0 / st->hyp[4] == 0.0)
        return fit_fail(BN_ERR_INVALID, "the raw parameters give an outputscale, lengthscale or noise out of range");
    return BN_OK;
}

int fit_upload_state(bn_gp_fit *h, const GpFitState &st)
{
    FIT_HIP(hipStreamSynchronize(h->last));
    FIT_HIP(hipMemcpy(h->st, &st, sizeof(st), hipMemcpyHostToDevice));
    return BN_OK;
}

int fit_download_state(bn_gp_fit *h, GpFitState *st)
{
    FIT_HIP(hipStreamSynchronize(h->last));
    FIT_HIP(hipMemcpy(st, h->st, sizeof(*st), hipMemcpyDeviceToHost));
    return BN_OK;
}

}  // namespace
}  // namespace bn

using bn::fit_fail;

extern "C" {

const char *bn_gp_fit_last_error(void) { return bn::g_fit_error.c_str(); }

size_t bn_gp_fit_workspace_bytes(int32_t n)
{
    if (n < 1 || n > bn::kFitMaxPoints) return 0;
    const size_t np = (size_t)bn::fit_npad(n), T = np / bn::kFitNB;
    return 2 * np * np * 8 + T * bn::kFitTile * 8 + 4 * np * 8 + 3 * (T * (T + 1) / 2) * 8 + (size_t)bn::kFitHistory * 8 + sizeof(bn::GpFitState);
}

int bn_gp_fit_create(int32_t device_id, int32_t n, const double *x, const double *y, double noise_lower_bound, bn_gp_fit_t **out)
{
    if (!out) return fit_fail(BN_ERR_INVALID, "null handle pointer");
    *out = nullptr;
    if (!x || !y) return fit_fail(BN_ERR_INVALID, "null argument");
    if (n < 1 || n > bn::kFitMaxPoints) return fit_fail(BN_ERR_INVALID, "n must be in [1, " + std::to_string(bn::kFitMaxPoints) + "] training points");
    if (!std::isfinite(noise_lower_bound) || noise_lower_bound < 0.0) return fit_fail(BN_ERR_INVALID, "noise_lower_bound must be finite and >= 0");
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(x[i]) || !std::isfinite(y[i])) return fit_fail(BN_ERR_INVALID, "x and y must be finite");
    if (int rc = bn::open_device(device_id, fit_fail)) return rc;
    BN_ON_DEVICE(fit_fail, device_id);
    auto *h = new bn_gp_fit_t();
    h->device = device_id; h->n = n; h->npad = bn::fit_npad(n); h->T = h->npad / bn::kFitNB;
    const size_t np = (size_t)h->npad, T = (size_t)h->T;
    h->bufs.add(&h->st, sizeof(bn::GpFitState));
    h->bufs.add(&h->x, np * 8);
    h->bufs.add(&h->y, np * 8);
    h->bufs.add(&h->A, np * np * 8);
    h->bufs.add(&h->X, np * np * 8);
    h->bufs.add(&h->dinv, T * bn::kFitTile * 8);
    h->bufs.add(&h->z, np * 8);
    h->bufs.add(&h->alpha, np * 8);
    h->bufs.add(&h->part, 3 * (T * (T + 1) / 2) * 8);
    h->bufs.add(&h->history, (size_t)bn::kFitHistory * 8);
    int rc = h->bufs.alloc_all(fit_fail);
    if (rc == BN_OK) {
        hipError_t e = hipMemcpy(h->x, x, (size_t)n * 8, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(h->y, y, (size_t)n * 8, hipMemcpyHostToDevice);
        if (e != hipSuccess) rc = fit_fail(BN_ERR_HIP, std::string("hipMemcpy: ") + hipGetErrorString(e));
    }
    if (rc == BN_OK) {
        const double zero[4] = {0.0, 0.0, 0.0, 0.0};     // gpytorch's initial raw parameters
        bn::GpFitState st{};
        rc = bn::fit_state_from_raw(zero, noise_lower_bound, &st);
        if (rc == BN_OK) rc = bn::fit_upload_state(h, st);
    }
    if (rc != BN_OK) {
        bn_gp_fit_destroy(h);                // leaves the error text alone
        return rc;
    }
    *out = h;
    return BN_OK;
}

void bn_gp_fit_destroy(bn_gp_fit_t *h)
{
    if (!h) return;
    bn::DeviceGuard guard(h->device);
    (void)hipStreamSynchronize(h->last);
    h->bufs.free_all();
    delete h;
}

int bn_gp_fit_set_raw(bn_gp_fit_t *h, const double *raw)
{
    if (!h || !raw) return fit_fail(BN_ERR_INVALID, "null argument");
    for (int p = 0; p < 4; ++p)
        if (!std::isfinite(raw[p])) return fit_fail(BN_ERR_INVALID, "the raw parameters must be finite");
    BN_ON_DEVICE(fit_fail, h->device);
    bn::GpFitState old{}, st{};
    if (int rc = bn::fit_download_state(h, &old)) return rc;
    if (int rc = bn::fit_state_from_raw(raw, old.lower_bound, &st)) return rc;
    h->enqueued = 0;                      // a new start: moments, history, status and iteration count are cleared
    return bn::fit_upload_state(h, st);
}

int bn_gp_fit_set_hyperparameters(bn_gp_fit_t *h, double constant, double outputscale, double lengthscale, double noise)
{
    if (!h) return fit_fail(BN_ERR_INVALID, "null argument");
    if (!std::isfinite(constant) || !std::isfinite(outputscale) || !std::isfinite(lengthscale) || !std::isfinite(noise))
        return fit_fail(BN_ERR_INVALID, "constant, outputscale, lengthscale and noise must be finite");
    if (!(outputscale > 0.0) || !(lengthscale > 0.0) || !(noise > 0.0)) return fit_fail(BN_ERR_INVALID, "outputscale, lengthscale and noise must be > 0");
    const double q = -1.0 / (2.0 * lengthscale * lengthscale);
    if (!std::isfinite(q) || q == 0.0) return fit_fail(BN_ERR_INVALID, "lengthscale out of range: 1 / (2 l^2) must be finite and non-zero");
    BN_ON_DEVICE(fit_fail, h->device);
    bn::GpFitState old{}, st{};
    if (int rc = bn::fit_download_state(h, &old)) return rc;
    st.lower_bound = old.lower_bound;
    for (int p = 0; p < 4; ++p) st.raw[p] = NAN;         // no raw parameters stand behind these values
    st.hyp[0] = constant; st.hyp[1] = outputscale; st.hyp[2] = lengthscale; st.hyp[3] = noise; st.hyp[4] = 2.0 * lengthscale * lengthscale;
    h->enqueued = 0;
    return bn::fit_upload_state(h, st);
}

int bn_gp_fit_evaluate_async(bn_gp_fit_t *h, void *stream)
{
    if (!h) return fit_fail(BN_ERR_INVALID, "null argument");
    BN_ON_DEVICE(fit_fail, h->device);
    return bn::fit_enqueue(h, (hipStream_t)stream, true);
}

int bn_gp_fit_run_async(bn_gp_fit_t *h, void *stream, int32_t iterations, double lr, double beta1, double beta2, double eps)
{
    if (iterations < 0) return fit_fail(BN_ERR_INVALID, "iterations must be >= 0");
    if (!(lr > 0.0) || !std::isfinite(lr)) return fit_fail(BN_ERR_INVALID, "lr must be finite and > 0");
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return fit_fail(BN_ERR_INVALID, "beta1 and beta2 must be in [0, 1)");
    if (!(eps >= 0.0) || !std::isfinite(eps)) return fit_fail(BN_ERR_INVALID, "eps must be finite and >= 0");
    if (!h) return fit_fail(BN_ERR_INVALID, "null argument");
    if (h->enqueued + (int64_t)iterations > bn::kFitHistory)
        return fit_fail(BN_ERR_INVALID, "a handle records at most " + std::to_string(bn::kFitHistory) + " iterations");
    BN_ON_DEVICE(fit_fail, h->device);
    hipStream_t s = (hipStream_t)stream;
    for (int it = 0; it < iterations; ++it) {
        if (int rc = bn::fit_enqueue(h, s, true)) return rc;
        bn::gp_fit_adam_kernel<<<1, 1, 0, s>>>(h->st, h->history, bn::kFitHistory, lr, beta1, beta2, eps);
        ++h->enqueued;
    }
    FIT_HIP(hipGetLastError());
    h->last = s;
    return BN_OK;
}

int bn_gp_fit_read(bn_gp_fit_t *h, double *raw, double *grad, double *loss, int32_t *status, int32_t *failed_iteration)
{
    if (!h) return fit_fail(BN_ERR_INVALID, "null argument");
    BN_ON_DEVICE(fit_fail, h->device);
    bn::GpFitState st{};
    if (int rc = bn::fit_download_state(h, &st)) return rc;
    if (raw) std::memcpy(raw, st.raw, sizeof(st.raw));
    if (grad) std::memcpy(grad, st.grad, sizeof(st.grad));
    if (loss) *loss = st.loss;
    if (status) *status = st.status;
    if (failed_iteration) *failed_iteration = st.status ? st.failed_iteration : -1;
    return BN_OK;
}

int bn_gp_fit_hyperparameters(bn_gp_fit_t *h, double *hyp)
{
    if (!h || !hyp) return fit_fail(BN_ERR_INVALID, "null argument");
    BN_ON_DEVICE(fit_fail, h->device);
    bn::GpFitState st{};
    if (int rc = bn::fit_download_state(h, &st)) return rc;
    std::memcpy(hyp, st.hyp, 4 * sizeof(double));
    return BN_OK;
}

int32_t bn_gp_fit_history(bn_gp_fit_t *h, double *losses, int32_t capacity)
{
    if (!h || (!losses && capacity > 0) || capacity < 0) return fit_fail(BN_ERR_INVALID, "null argument or negative capacity");
    BN_ON_DEVICE(fit_fail, h->device);
    bn::GpFitState st{};
    if (int rc = bn::fit_download_state(h, &st)) return rc;
    const int done = st.iteration < bn::kFitHistory ? st.iteration : bn::kFitHistory;
    const int k = done < capacity ? done : capacity;
    if (k > 0) FIT_HIP(hipMemcpy(losses, h->history, (size_t)k * 8, hipMemcpyDeviceToHost));
    return done;
}

int bn_gp_fit_finish(bn_gp_fit_t *h, void *stream, bn_gp_t **out)
{
    if (!out) return fit_fail(BN_ERR_INVALID, "null handle pointer");
    *out = nullptr;
    if (!h) return fit_fail(BN_ERR_INVALID, "null argument");
    BN_ON_DEVICE(fit_fail, h->device);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = bn::fit_enqueue(h, s, false)) return rc;
    bn::GpFitState st{};
    if (int rc = bn::fit_download_state(h, &st)) return rc;
    if (st.status)
        return fit_fail(BN_ERR_STATE, "k(x, x) + noise I is not numerically positive definite at iteration " + std::to_string(st.failed_iteration) +
                                          " (no jitter is added)");
    auto *g = new bn_gp_t();
    g->device = h->device; g->n = h->n;
    g->c = st.hyp[0]; g->s = st.hyp[1]; g->l = st.hyp[2]; g->noise = st.hyp[3];
    bn::gp_layout(g);
    const int nb = g->npad / 16;
    int rc = g->bufs.alloc_all(fit_fail);
    if (rc == BN_OK) {
        // the padded x and alpha of the fit are zero beyond n, and npad of the handle is <= the fit's
        hipError_t e = hipMemcpyAsync(g->x, h->x, (size_t)g->npad * 8, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(g->alpha, h->alpha, (size_t)g->npad * 8, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) {
            bn::gp_fit_pack_kernel<<<dim3(nb, nb), 256, 0, s>>>(h->dev(), g->linv);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) rc = fit_fail(BN_ERR_HIP, std::string("bn_gp_fit_finish: ") + hipGetErrorString(e));
    }
    if (rc != BN_OK) {
        g->bufs.free_all();
        delete g;
        return rc;
    }
    *out = g;
    return BN_OK;
}

}  // extern "C"
