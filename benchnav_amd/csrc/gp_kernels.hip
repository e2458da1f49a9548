// gp_kernels.hip -- exact-GP slip prediction: TraversabilityPredictor.predict's per-class GP regressors
// (src/prediction_models/traversability_predictors/classifier_and_regressor.py:42-72, slip_regressors/gpr.py) for B maps.
//
//   k(a, b) = s exp(-(a - b)^2 / (2 l^2)),  K = k(x, x) + noise I = L L^T,  alpha = K^-1 (y - c)
//   mean(phi) = c + k(phi, x) . alpha,  v = L^-1 k(x, phi),  std(phi) = sqrt(max(s - |v|^2, 0) + noise)
//
// All of it in float64; the outputs alone are rounded to float32 (the variance is a difference of nearly equal numbers).
// Two launches per call, no host round trip:
//   gp_bucket_kernel    one workgroup per map sorts the map's cells by class into an index list, with the count, the list offset
//                       and the first tile of every class; the cells without a regressor get 0 / 0 here.
//   gp_predict_kernel   N <= 1024: one workgroup per tile of 16 cells of one class: the k(x, phi) columns into LDS, then
//                       v = L^-1 k on v_mfma_f64_16x16x4_f64 over the blocks on and below the diagonal, |v|^2 and k . alpha
//                       reduced per column.
//   gp_slab_kernel      N > 1024 (up to 10240): one workgroup per four consecutive tiles (64 cells) of one class walks L^-1 in
//                       slabs of 32 row blocks and regenerates k(x, phi) in chunks of 128 points per slab (the whole k does not
//                       fit the LDS); every fragment of L^-1 feeds four MFMAs.
// A call launches the bucketing and whichever of the two predict kernels its regressors need (two or three launches).
// Every sum runs in an order fixed by N alone: a cell's result does not depend on the tile, column or map it lands in.
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

constexpr int kGpSmallMax = 1024;        // gp_predict_kernel: the k tile of 16 cells x 1024 points x 8 bytes is 128 KB of the CU's 160 KB of LDS
constexpr int kGpMaxPoints = 10240;      // gp_slab_kernel: 640 row blocks, 420 MB of L^-1 fragments
constexpr int kGpMaxClasses = 32;
constexpr int kGpTile = 16;              // cells per tile: the N of the MFMA
constexpr int kGpWaves = 8;
constexpr int kGpThreads = kGpWaves * 64;
constexpr int kGpGroups = kGpThreads / kGpTile;   // point groups of the generation phase
constexpr int kGpBucketThreads = 1024;

using f64x4 = __attribute__((ext_vector_type(4))) double;

struct GpTable {
    GpRegDev r[kGpMaxClasses];
};

// per map: count[C], list offset[C], first tile[C + 1]
__host__ __device__ inline int gp_meta_stride(int C) { return 3 * C + 1; }

struct GpBucketArgs {
    const int32_t *classes;              // (B, cells)
    int32_t *idx;                        // (B, cells) cell indices sorted by class
    int32_t *meta;                       // (B, gp_meta_stride(C))
    void *mean, *std;                    // (B, cells)
    int32_t cells, C, f64;
    uint32_t present;                    // bit c: class c has a regressor
};

__global__ __launch_bounds__(kGpBucketThreads) void gp_bucket_kernel(GpBucketArgs a)
{
    __shared__ int cnt[kGpMaxClasses], cur[kGpMaxClasses];
    const int t = threadIdx.x, lane = t & 63, b = blockIdx.x;
    const size_t base = (size_t)b * a.cells;
    const int32_t *cls = a.classes + base;
    if (t < kGpMaxClasses) cnt[t] = 0;
    __syncthreads();
    const int rounds = (a.cells + kGpBucketThreads - 1) / kGpBucketThreads;
    for (int it = 0; it < rounds; ++it) {
        const int cell = it * kGpBucketThreads + t;
        int c = -1;
        if (cell < a.cells) {
            c = cls[cell];
            if (c < 0 || c >= a.C || !((a.present >> c) & 1u)) c = -1;
        }
        for (int k = 0; k < a.C; ++k) {
            if (!((a.present >> k) & 1u)) continue;
            const unsigned long long m = __ballot(c == k);
            if (lane == 0 && m) atomicAdd(&cnt[k], __popcll(m));
        }
    }
    __syncthreads();
    if (t == 0) {
        int32_t *meta = a.meta + (size_t)b * gp_meta_stride(a.C);
        int s = 0, ts = 0;
        for (int k = 0; k < a.C; ++k) {
            cur[k] = s;
            meta[k] = cnt[k];
            meta[a.C + k] = s;
            meta[2 * a.C + k] = ts;
            s += cnt[k];
            ts += (cnt[k] + kGpTile - 1) / kGpTile;
        }
        meta[3 * a.C] = ts;
    }
    __syncthreads();
    int32_t *idx = a.idx + base;
    for (int it = 0; it < rounds; ++it) {
        const int cell = it * kGpBucketThreads + t;
        int c = -1;
        if (cell < a.cells) {
            c = cls[cell];
            if (c < 0 || c >= a.C || !((a.present >> c) & 1u)) c = -1;
            if (c < 0) {                 // no regressor: the reference's zeros_like
                if (a.f64) { ((double *)a.mean)[base + cell] = 0.0; ((double *)a.std)[base + cell] = 0.0; }
                else { ((float *)a.mean)[base + cell] = 0.0f; ((float *)a.std)[base + cell] = 0.0f; }
            }
        }
        for (int k = 0; k < a.C; ++k) {
            if (!((a.present >> k) & 1u)) continue;
            const unsigned long long m = __ballot(c == k);
            if (!m) continue;
            int at = 0;
            if (lane == 0) at = atomicAdd(&cur[k], __popcll(m));
            at = __shfl(at, 0);
            if (c == k) idx[at + __popcll(m & ((1ull << lane) - 1ull))] = cell;
        }
    }
}

struct GpPredictArgs {
    GpTable table;
    const float *slopes;                 // (B, cells)
    const int32_t *idx, *meta;
    void *mean, *std;
    int32_t cells, C, f64;
};

__device__ __forceinline__ f64x4 gp_mfma(double a, double b, f64x4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// LDS: kt[npad][16] the k(x, phi) tile (point-major: step j of the MFMA's B operand is the 64 consecutive doubles at 64 j),
// then mean_part[kGpGroups][16] and sq_part[kGpWaves][64].
__global__ __launch_bounds__(kGpThreads) void gp_predict_kernel(GpPredictArgs a)
{
    extern __shared__ double gp_lds[];
    const int t = threadIdx.x, b = blockIdx.y, tile = blockIdx.x;
    const int32_t *meta = a.meta + (size_t)b * gp_meta_stride(a.C);
    if (tile >= meta[3 * a.C]) return;
    int c = 0;
    for (int k = 0; k < a.C; ++k)
        if (tile >= meta[2 * a.C + k] && tile < meta[2 * a.C + k + 1]) c = k;
    const int first = (tile - meta[2 * a.C + c]) * kGpTile;
    const int ncell = min(kGpTile, meta[c] - first);
    const size_t base = (size_t)b * a.cells;
    const int32_t *idx = a.idx + base + meta[a.C + c] + first;
    const GpRegDev *rp = &a.table.r[c];
    if (rp->npad > kGpSmallMax) return;  // gp_slab_kernel's class
    const double *x = rp->x, *alpha = rp->alpha, *linv = rp->linv;
    const int n = rp->n, npad = rp->npad;
    const double gc = rp->c, gs = rp->s, gq = rp->q, gnoise = rp->noise;
    double *kt = gp_lds, *mean_part = kt + (size_t)npad * kGpTile, *sq_part = mean_part + kGpGroups * kGpTile;

    {   // the k tile, and k . alpha per (point group, cell): group g sums its points p = g, g + 32, ... in order
        const int cc = t & (kGpTile - 1), g = t / kGpTile;
        const double phi = cc < ncell ? (double)a.slopes[base + idx[cc]] : 0.0;
        double msum = 0.0;
        for (int p = g; p < npad; p += kGpGroups) {
            double kv = 0.0;
            if (p < n) {
                const double d = phi - x[p];
                kv = gs * exp((d * d) * gq);
                msum = __builtin_fma(kv, alpha[p], msum);
            }
            kt[p * kGpTile + cc] = kv;
        }
        mean_part[g * kGpTile + cc] = msum;
    }
    __syncthreads();

    {   // v = L^-1 k: wave w takes the row-block pairs (p, nb - 1 - p), p = w, w + 8, ...: every pair is nb + 1 blocks of work.
        // The accumulator of a row block sums over k in ascending order; C/D of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 r.
        const int w = __builtin_amdgcn_readfirstlane(t >> 6), l = t & 63;
        const int nb = npad / kGpTile, npairs = (nb + 1) / 2;
        double sq = 0.0;
        for (int p = w; p < npairs; p += kGpWaves) {
            const int i0 = p, i1 = nb - 1 - p;
            const bool two = i1 != i0;
            const int steps0 = two ? 4 * (i0 + 1) : 0, steps1 = 4 * (i1 + 1);
            const double *A0 = linv + (size_t)128 * i0 * (i0 + 1) + l, *A1 = linv + (size_t)128 * i1 * (i1 + 1) + l;
            f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
            // the next four steps' fragments are always in flight behind the current ones (loads past a row block's end repeat
            // its last four steps: unconditional loads let the wait for the current fragments leave the next ones outstanding)
            const int last1 = steps1 - 4, last0 = steps0 > 4 ? steps0 - 4 : 0;
            double a1[4], a0[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { a1[u] = A1[64 * u]; a0[u] = A0[64 * u]; }
            for (int j = 0; j < steps1; j += 4) {
                const int j1 = min(j + 4, last1), j0 = min(j + 4, last0);
                double n1[4], n0[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) { n1[u] = A1[64 * (j1 + u)]; n0[u] = A0[64 * (j0 + u)]; }
                double bk[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) bk[u] = kt[64 * (j + u) + l];
#pragma unroll
                for (int u = 0; u < 4; ++u) acc1 = gp_mfma(a1[u], bk[u], acc1);
                if (j < steps0) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) acc0 = gp_mfma(a0[u], bk[u], acc0);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) { a1[u] = n1[u]; a0[u] = n0[u]; }
            }
            if (two) {
#pragma unroll
                for (int r = 0; r < 4; ++r) sq = __builtin_fma(acc0[r], acc0[r], sq);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) sq = __builtin_fma(acc1[r], acc1[r], sq);
        }
        sq_part[t] = sq;
    }
    __syncthreads();

    if (t < ncell) {
        double tot = 0.0, m = 0.0;
        for (int k = 0; k < kGpWaves * 4; ++k) tot += sq_part[k * kGpTile + t];
        for (int g = 0; g < kGpGroups; ++g) m += mean_part[g * kGpTile + t];
        const double mean = gc + m;
        const double sd = sqrt(fmax(gs - tot, 0.0) + gnoise);
        const size_t o = base + idx[t];
        if (a.f64) { ((double *)a.mean)[o] = mean; ((double *)a.std)[o] = sd; }
        else { ((float *)a.mean)[o] = (float)mean; ((float *)a.std)[o] = (float)sd; }
    }
}

// ---- N > 1024 ----
constexpr int kSlabTiles = 4;                             // tiles per workgroup
constexpr int kSlabCells = kSlabTiles * kGpTile;          // 64 cells: every fragment of L^-1 feeds four MFMAs
constexpr int kSlabChunkBlocks = 8;                       // k blocks (of 16 points) per chunk
constexpr int kSlabChunk = kSlabChunkBlocks * kGpTile;    // 128 points: two chunks of 64 cells are 128 KB of LDS
constexpr int kSlabRb = 4;                                // row blocks per wave and slab: 16 accumulators of 4 doubles, 128 registers
constexpr int kSlabBlocks = kGpWaves * kSlabRb;           // 32 row blocks (512 rows) per slab

constexpr size_t gp_slab_lds() { return (size_t)2 * kSlabChunk * kSlabCells * sizeof(double); }

// One workgroup per group of four consecutive tiles of a class with more than kGpSmallMax points (the bucket kernel's tile
// numbering: the workgroup of the group's first tile works, the other three return).  L^-1 is walked in slabs of 32 row blocks;
// in slab s wave w owns the row blocks 32 s + w + 8 r, r < 4, with four accumulators (one per tile) each.  For every slab the
// workgroup walks the k chunks from 0 to the slab's last column in ascending order: chunk ch + 1 is generated into one half of
// the LDS while chunk ch is consumed from the other (waves 0-3 generate first, waves 4-7 consume first, so that the two waves
// of a SIMD overlap exp and MFMA work), one barrier per chunk.  A row block's accumulator sums over k in ascending order, as in
// gp_predict_kernel; at the slab's end every lane folds its 64 values into four running sums of |v|^2 (one per tile) in the
// order row block, register.  k . alpha is accumulated in the last slab alone, which passes over every chunk.
// LDS: kt[2][tile][128 points][16 cells]; after the last slab the same memory takes sq_part[wave][tile][64] and mean_part[8][64].
__global__ __launch_bounds__(kGpThreads) void gp_slab_kernel(GpPredictArgs a)
{
    extern __shared__ double gp_lds[];
    const int t = threadIdx.x, b = blockIdx.y, tile = blockIdx.x;
    const int32_t *meta = a.meta + (size_t)b * gp_meta_stride(a.C);
    if (tile >= meta[3 * a.C]) return;
    int c = 0;
    for (int k = 0; k < a.C; ++k)
        if (tile >= meta[2 * a.C + k] && tile < meta[2 * a.C + k + 1]) c = k;
    const int tl = tile - meta[2 * a.C + c];
    const GpRegDev *rp = &a.table.r[c];
    if (rp->npad <= kGpSmallMax || (tl & (kSlabTiles - 1))) return;
    const int first = tl * kGpTile;
    const int ncell = min(kSlabCells, meta[c] - first);
    const size_t base = (size_t)b * a.cells;
    const int32_t *idx = a.idx + base + meta[a.C + c] + first;
    const double *x = rp->x, *alpha = rp->alpha, *linv = rp->linv;
    const int n = rp->n, nb = rp->npad / kGpTile;
    const double gc = rp->c, gs = rp->s, gq = rp->q, gnoise = rp->noise;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6), l = t & 63;
    const int nslabs = (nb + kSlabBlocks - 1) / kSlabBlocks;

    // generation: thread (w, l) takes cell l and the points w, w + 8, ... of the chunk
    const double phi = l < ncell ? (double)a.slopes[base + idx[l]] : 0.0;
    double *kcol = gp_lds + (size_t)(l >> 4) * kSlabChunk * kGpTile + (l & 15);
    double msum = 0.0;
    auto generate = [&](int ch, int half, bool with_mean) {
        double *dst = kcol + (size_t)half * kSlabChunk * kSlabCells;
        const int p0 = ch * kSlabChunk;
#pragma unroll 4
        for (int m = 0; m < kSlabChunk / kGpWaves; ++m) {
            const int pl = w + kGpWaves * m, p = p0 + pl;
            double kv = 0.0;
            if (p < n) {
                const double d = phi - x[p];
                kv = gs * exp((d * d) * gq);
                if (with_mean) msum = __builtin_fma(kv, alpha[p], msum);
            }
            dst[pl * kGpTile] = kv;
        }
    };

    double sq[kSlabTiles] = {0.0, 0.0, 0.0, 0.0};
    for (int s = 0; s < nslabs; ++s) {
        const bool last = s == nslabs - 1;
        int iv[kSlabRb];                 // the wave's row blocks, -1 beyond the matrix
        const double *A[kSlabRb];
#pragma unroll
        for (int r = 0; r < kSlabRb; ++r) {
            const int i = s * kSlabBlocks + w + kGpWaves * r;
            iv[r] = i < nb ? i : -1;
            A[r] = linv + (size_t)128 * (i < nb ? i : 0) * ((i < nb ? i : 0) + 1) + l;
        }
        const int imin = iv[kSlabRb - 1] < 0 ? -1 : iv[0];       // k blocks 0 ... imin take all four row blocks
        const int imax = max(max(iv[0], iv[1]), max(iv[2], iv[3]));
        const int kbend = min((s + 1) * kSlabBlocks, nb);
        const int nch = (kbend + kSlabChunkBlocks - 1) / kSlabChunkBlocks;
        f64x4 acc[kSlabRb][kSlabTiles];
#pragma unroll
        for (int r = 0; r < kSlabRb; ++r)
#pragma unroll
            for (int q = 0; q < kSlabTiles; ++q) acc[r][q] = f64x4{0.0, 0.0, 0.0, 0.0};
        // the fragments of the next k block are in flight behind the current ones, across chunks too
        double an[kSlabRb][4];
#pragma unroll
        for (int r = 0; r < kSlabRb; ++r)
#pragma unroll
            for (int u = 0; u < 4; ++u) an[r][u] = imin >= 0 ? A[r][64 * u] : 0.0;

        generate(0, 0, last);
        __syncthreads();
        for (int ch = 0; ch < nch; ++ch) {
            const bool more = ch + 1 < nch;
            if (w < kGpWaves / 2 && more) generate(ch + 1, (ch + 1) & 1, last);
            {
                const double *kt = gp_lds + (size_t)(ch & 1) * kSlabChunk * kSlabCells + l;
                const int kb0 = ch * kSlabChunkBlocks, kb1 = min(kb0 + kSlabChunkBlocks, kbend);
                const int full1 = min(kb1, imin + 1);
                for (int kb = kb0; kb < full1; ++kb) {
                    const int kn = min(kb + 1, imin);    // at the last full k block the reload repeats it: the loads stay unconditional
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        double bk[kSlabTiles];
#pragma unroll
                        for (int q = 0; q < kSlabTiles; ++q) bk[q] = kt[q * kSlabChunk * kGpTile + 64 * (4 * (kb - kb0) + u)];
#pragma unroll
                        for (int r = 0; r < kSlabRb; ++r)
#pragma unroll
                            for (int q = 0; q < kSlabTiles; ++q) acc[r][q] = gp_mfma(an[r][u], bk[q], acc[r][q]);
                        // step u's fragments of the next k block go into the registers that step u has just read: 48 MFMAs ahead
#pragma unroll
                        for (int r = 0; r < kSlabRb; ++r) an[r][u] = A[r][64 * (4 * kn + u)];
                    }
                }
                // around the diagonal (and in a last slab with fewer than four row blocks for the wave): row block by row block
                const int diag1 = min(kb1, imax + 1);
                for (int kb = max(kb0, imin + 1); kb < diag1; ++kb) {
#pragma unroll
                    for (int r = 0; r < kSlabRb; ++r) {
                        if (kb > iv[r]) continue;
                        double ac[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) ac[u] = A[r][64 * (4 * kb + u)];
#pragma unroll
                        for (int u = 0; u < 4; ++u)
#pragma unroll
                            for (int q = 0; q < kSlabTiles; ++q)
                                acc[r][q] = gp_mfma(ac[u], kt[q * kSlabChunk * kGpTile + 64 * (4 * (kb - kb0) + u)], acc[r][q]);
                    }
                }
            }
            if (w >= kGpWaves / 2 && more) generate(ch + 1, (ch + 1) & 1, last);
            __syncthreads();
        }
#pragma unroll
        for (int r = 0; r < kSlabRb; ++r)
#pragma unroll
            for (int q = 0; q < kSlabTiles; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) sq[q] = __builtin_fma(acc[r][q][e], acc[r][q][e], sq[q]);
    }

    // every wave is past the last chunk's barrier: the k memory is free
    double *sq_part = gp_lds, *mean_part = gp_lds + kGpWaves * kSlabTiles * 64;
#pragma unroll
    for (int q = 0; q < kSlabTiles; ++q) sq_part[(w * kSlabTiles + q) * 64 + l] = sq[q];
    mean_part[w * kSlabCells + l] = msum;
    __syncthreads();
    if (t < ncell) {
        const int q = t >> 4, col = t & 15;
        double tot = 0.0, m = 0.0;
        for (int k = 0; k < kGpWaves; ++k)
            for (int g = 0; g < 4; ++g) tot += sq_part[(k * kSlabTiles + q) * 64 + 16 * g + col];
        for (int g = 0; g < kGpWaves; ++g) m += mean_part[g * kSlabCells + t];
        const double mean = gc + m;
        const double sd = sqrt(fmax(gs - tot, 0.0) + gnoise);
        const size_t o = base + idx[t];
        if (a.f64) { ((double *)a.mean)[o] = mean; ((double *)a.std)[o] = sd; }
        else { ((float *)a.mean)[o] = (float)mean; ((float *)a.std)[o] = (float)sd; }
    }
}

size_t gp_predict_lds(int npad) { return ((size_t)npad * kGpTile + kGpGroups * kGpTile + kGpThreads) * sizeof(double); }

thread_local std::string g_gp_error;

int gp_fail(int code, const std::string &msg)
{
    g_gp_error = msg;
    return code;
}

#define GP_HIP(expr) BN_HIP_AS(gp_fail, expr, #expr)

size_t gp_align(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace
}  // namespace bn

using bn::gp_fail;

extern "C" {

const char *bn_gp_last_error(void) { return bn::g_gp_error.c_str(); }

int32_t bn_gp_max_points(void) { return bn::kGpMaxPoints; }

int bn_gp_create(int32_t device_id, int32_t n, const double *x, const double *alpha, const double *linv, double constant,
                 double outputscale, double lengthscale, double noise, bn_gp_t **out)
{
    if (!out) return gp_fail(BN_ERR_INVALID, "null handle pointer");
    *out = nullptr;
    if (!x || !alpha || !linv) return gp_fail(BN_ERR_INVALID, "null argument");
    if (n < 1 || n > bn::kGpMaxPoints) return gp_fail(BN_ERR_INVALID, "n must be in [1, " + std::to_string(bn::kGpMaxPoints) + "] training points");
    if (!std::isfinite(constant) || !std::isfinite(outputscale) || !std::isfinite(lengthscale) || !std::isfinite(noise))
        return gp_fail(BN_ERR_INVALID, "constant, outputscale, lengthscale and noise must be finite");
    if (!(outputscale > 0.0) || !(lengthscale > 0.0) || !(noise > 0.0)) return gp_fail(BN_ERR_INVALID, "outputscale, lengthscale and noise must be > 0");
    const double q = -1.0 / (2.0 * lengthscale * lengthscale);
    if (!std::isfinite(q) || q == 0.0) return gp_fail(BN_ERR_INVALID, "lengthscale out of range: 1 / (2 l^2) must be finite and non-zero");
    for (size_t i = 0; i < (size_t)n; ++i) {
        if (!std::isfinite(x[i]) || !std::isfinite(alpha[i])) return gp_fail(BN_ERR_INVALID, "x and alpha must be finite");
        for (size_t j = 0; j <= i; ++j)
            if (!std::isfinite(linv[i * (size_t)n + j])) return gp_fail(BN_ERR_INVALID, "the lower triangle of linv must be finite");
    }
    if (int rc = bn::open_device(device_id, gp_fail)) return rc;
    BN_ON_DEVICE(gp_fail, device_id);
    auto *h = new bn_gp_t();
    h->device = device_id; h->n = n;
    h->c = constant; h->s = outputscale; h->l = lengthscale; h->noise = noise;
    const size_t nfrag = bn::gp_layout(h);
    const int npad = h->npad, nb = npad / bn::kGpTile;
    // L^-1 in the order the MFMA's A operand is read: row block i, k step j, lane -> L^-1[16 i + (lane & 15)][4 j + (lane >> 4)]
    std::vector<double> xs(npad, 0.0), as(npad, 0.0), frag(nfrag, 0.0);
    std::memcpy(xs.data(), x, (size_t)n * 8);
    std::memcpy(as.data(), alpha, (size_t)n * 8);
    for (int i = 0; i < nb; ++i)
        for (int j = 0; j < 4 * (i + 1); ++j) {
            double *f = frag.data() + (size_t)128 * i * (i + 1) + (size_t)64 * j;
            for (int l = 0; l < 64; ++l) {
                const int row = 16 * i + (l & 15), col = 4 * j + (l >> 4);
                f[l] = (row < n && col <= row) ? linv[(size_t)row * n + col] : 0.0;
            }
        }
    int rc = h->bufs.alloc_all(gp_fail);
    if (rc == BN_OK) {
        auto up = [&](void *dst, const std::vector<double> &src) {
            hipError_t e = hipMemcpy(dst, src.data(), src.size() * 8, hipMemcpyHostToDevice);
            return e == hipSuccess ? BN_OK : gp_fail(BN_ERR_HIP, std::string("hipMemcpy: ") + hipGetErrorString(e));
        };
        if ((rc = up(h->x, xs)) == BN_OK && (rc = up(h->alpha, as)) == BN_OK) rc = up(h->linv, frag);
    }
    if (rc != BN_OK) {
        bn_gp_destroy(h);                    // leaves the error text alone
        return rc;
    }
    *out = h;
    return BN_OK;
}

void bn_gp_destroy(bn_gp_t *h)
{
    if (!h) return;
    bn::DeviceGuard guard(h->device);
    h->bufs.free_all();
    delete h;
}

size_t bn_gp_workspace_bytes(int32_t num_maps, int64_t cells, int32_t num_classes)
{
    if (num_maps < 1 || cells < 1 || num_classes < 1 || num_classes > bn::kGpMaxClasses) return 0;
    return bn::gp_align((size_t)num_maps * (size_t)cells * 4) + bn::gp_align((size_t)num_maps * bn::gp_meta_stride(num_classes) * 4);
}

int bn_gp_predict_async(int32_t device_id, void *stream, bn_gp_t *const *regressors, int32_t num_classes, int32_t num_maps,
                        int64_t cells, const float *slopes_device, const int32_t *classes_device, void *mean_device,
                        void *std_device, int32_t f64_outputs, void *workspace_device, size_t workspace_bytes)
{
    if (!regressors || !slopes_device || !classes_device || !mean_device || !std_device || !workspace_device)
        return gp_fail(BN_ERR_INVALID, "null argument");
    if (num_classes < 1 || num_classes > bn::kGpMaxClasses)
        return gp_fail(BN_ERR_INVALID, "num_classes must be in [1, " + std::to_string(bn::kGpMaxClasses) + "]");
    if (num_maps < 1 || num_maps > 65535) return gp_fail(BN_ERR_INVALID, "num_maps must be in [1, 65535]");
    if (cells < 1 || cells > ((int64_t)1 << 30)) return gp_fail(BN_ERR_INVALID, "cells per map must be in [1, 2^30]");
    if (f64_outputs != 0 && f64_outputs != 1) return gp_fail(BN_ERR_INVALID, "f64_outputs must be 0 or 1");
    if (workspace_bytes < bn_gp_workspace_bytes(num_maps, cells, num_classes))
        return gp_fail(BN_ERR_INVALID, "workspace smaller than bn_gp_workspace_bytes(num_maps, cells, num_classes)");
    bn::GpPredictArgs p{};
    uint32_t present = 0;
    int npad_small = 0;
    bool large = false;
    for (int c = 0; c < num_classes; ++c) {
        const bn_gp_t *r = regressors[c];
        if (!r) continue;
        if (r->device != device_id) return gp_fail(BN_ERR_INVALID, "regressor " + std::to_string(c) + " lives on another device");
        present |= 1u << c;
        if (r->npad > bn::kGpSmallMax) large = true;
        else npad_small = r->npad > npad_small ? r->npad : npad_small;
        bn::GpRegDev &d = p.table.r[c];
        d.x = r->x; d.alpha = r->alpha; d.linv = r->linv; d.n = r->n; d.npad = r->npad;
        d.c = r->c; d.s = r->s; d.q = -1.0 / (2.0 * r->l * r->l); d.noise = r->noise;
    }
    if (int rc = bn::open_device(device_id, gp_fail)) return rc;
    BN_ON_DEVICE(gp_fail, device_id);
    hipStream_t s = (hipStream_t)stream;
    int32_t *idx = (int32_t *)workspace_device;
    int32_t *meta = (int32_t *)((char *)workspace_device + bn::gp_align((size_t)num_maps * (size_t)cells * 4));
    bn::GpBucketArgs g{};
    g.classes = classes_device; g.idx = idx; g.meta = meta; g.mean = mean_device; g.std = std_device;
    g.cells = (int32_t)cells; g.C = num_classes; g.f64 = f64_outputs; g.present = present;
    bn::gp_bucket_kernel<<<num_maps, bn::kGpBucketThreads, 0, s>>>(g);
    GP_HIP(hipGetLastError());
    if (!present) return BN_OK;
    p.slopes = slopes_device; p.idx = idx; p.meta = meta; p.mean = mean_device; p.std = std_device;
    p.cells = (int32_t)cells; p.C = num_classes; p.f64 = f64_outputs;
    // every class of a map ends in at most one partial tile; both kernels run over the same tile numbering and each leaves the
    // other's classes alone
    const unsigned tiles = (unsigned)((cells + bn::kGpTile - 1) / bn::kGpTile) + (unsigned)num_classes;
    if (npad_small) {
        const size_t lds = bn::gp_predict_lds(npad_small);       // sized by the largest class of this kernel
        GP_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(bn::gp_predict_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        bn::gp_predict_kernel<<<dim3(tiles, (unsigned)num_maps), bn::kGpThreads, lds, s>>>(p);
        GP_HIP(hipGetLastError());
    }
    if (large) {
        const size_t lds = bn::gp_slab_lds();
        GP_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(bn::gp_slab_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        bn::gp_slab_kernel<<<dim3(tiles, (unsigned)num_maps), bn::kGpThreads, lds, s>>>(p);
        GP_HIP(hipGetLastError());
    }
    return BN_OK;
}

}  // extern "C"
