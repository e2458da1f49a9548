// Terrain generation for B map instances of one grid size G (padded G' = G + 2): TerrainGeometry.set_terrain_geometry and
// TerrainTraversability.set_traversability of the reference (src/environments/terrain_properties.py) on the device.
//
// The draws come from the host (benchnav_amd/terrain.py replays the reference's CPU generator) or from
//   terrain_draws_kernel      one workgroup per instance: torch's MT19937 stream of the instance's seed in LDS, the crater rejection
//                             loop, the crater tables, the fBm phases and the light source, written where the kernels below read
// and the kernels do the arithmetic:
//   terrain_crater_kernel     one workgroup per instance, craters in order: carve the footprint (generate_crater :151-206),
//                             then the min-reduction and shift (adjust_height_values) -- float32 operations in the reference's order
//   terrain_spectrum_kernel   the final state of generate_fractal_surface's complex64 grid (:254-290), scaled (:293-295)
//   terrain_dft_rows_kernel   T = S W, W[l, x] = exp(+2 pi i l x / G'): the row pass of the inverse DFT, float64 accumulation
//   terrain_dft_cols_kernel   Re(W^T T) / G'^2, then the reference's float32 scaling, added to the padded heights (:296-299)
//   terrain_minshift_kernel   heights -= min(heights), one workgroup per instance
//   terrain_surface_kernel    crop, Horn slopes on the padded heights (generate_slopes :316-352), the per-class slip mean / std
//                             (slip_model.py model_mean / model_stddev; set_traversability :544-579)
// and, when colouring is set (TerrainColoring.set_terrain_class_coloring :364-523):
//   terrain_noise_kernel      the library's own seeded gradient noise (skipped when the caller uploads a field)
//   terrain_classes_kernel    ahead of the surface kernel: per-instance min / max, the normalised field against the occupancy
//                             thresholds -> the class map (generate_multi_terrain :421-443), and the two per-instance counters
//   terrain_color_kernel      after it: surface normals of the cropped heights, the light's shade on the class's colour
// Every index is bounded by the handle's G and B; crater slices are validated on the host and clamped here again.
// The host side takes its device guard and HIP check from bn_host.h; its buffers are reallocated as the draws and the colouring
// change size (realloc_dev), so they are not kept in that header's buffer table.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/benchnav_mppi.h"
#include "bn_device_math.h"
#include "bn_host.h"
#include "mt19937.h"

namespace bn {
namespace {

constexpr int kReduceThreads = 1024;
constexpr int kTile = 16;                  // DFT output tile (kTile x kTile threads) and reduction depth per LDS stage
constexpr int kMaxN = 1026;                // G' up to 1026 (G <= 1024): the twiddle table lives in LDS
constexpr int kClassParams = 6;            // present, f32(sens * 1e-3), nonlinearity, offset, base noise, slope noise

struct TerrainArgs {
    float *hp;                 // (B, N, N) padded heights
    float2 *S;                 // (B, N, N) scaled spectrum (complex64, as the reference's grid)
    double2 *T;                // (B, N, N) row pass
    const double2 *tw;         // (N) exp(+2 pi i m / N), host float64
    const float *phases;       // (B, nph)
    const int32_t *cr_count;   // (B)
    const int32_t *cr_int;     // (B, maxc, 8): sx, sy, ex, ey, psx, psy, n, lin offset
    const float *cr_val;       // (B, maxc, 2): f32 radius, f32 -tan(deg2rad(angle))
    const float *lin;          // profile coordinates of every crater
    const int32_t *classes;    // (B, G, G)
    const float *cparams;      // (C, kClassParams)
    float *heights, *slopes, *mean, *stddev;   // (B, G, G)
    int G, N, B, nph, maxc, lin_len, nclass;
    double expo;               // -(H + 1) / 2
    double scale;              // f32(|gain| * (N res 1e3)^(H + 1.5)) as a double
    float c_div;               // f32((res * 1e3)^2)
    float c_milli;             // f32(1e-3)
    double inv_8res;           // 1 / (8 res)
};

// the block's minimum of hp over one instance, then hp -= min (adjust_height_values): every thread returns after the shift
__device__ void block_min_shift(float *h, int cells, float *red)
{
    float m = INFINITY;
    for (int i = threadIdx.x; i < cells; i += blockDim.x) m = fminf(m, h[i]);
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = fminf(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    const float mn = red[0];
    __syncthreads();
    for (int i = threadIdx.x; i < cells; i += blockDim.x) h[i] = h[i] - mn;
    __syncthreads();
}

// generate_crater for every crater of instance blockIdx.x, in placement order, each followed by the min-shift.
// profile[i][j] = (-tan) * (r - sqrt(lin[i]^2 + lin[j]^2)) where the distance is <= r, else 0 ('ij' meshgrid: row i, column j);
// cells whose profile entry is non-zero get heights + profile (f32).
__global__ __launch_bounds__(kReduceThreads) void terrain_crater_kernel(TerrainArgs a)
{
    __shared__ float red[kReduceThreads];
    const int b = blockIdx.x;
    const int N = a.N, cells = N * N;
    float *h = a.hp + (size_t)b * cells;
    const int nc = a.cr_count[b];
    for (int c = 0; c < nc && c < a.maxc; ++c) {
        const int32_t *ci = a.cr_int + ((size_t)b * a.maxc + c) * 8;
        const int sx = max(ci[0], 0), sy = max(ci[1], 0), ex = min(ci[2], N), ey = min(ci[3], N);
        const int psx = ci[4], psy = ci[5], n = ci[6], off = ci[7];
        const float r = a.cr_val[((size_t)b * a.maxc + c) * 2], nt = a.cr_val[((size_t)b * a.maxc + c) * 2 + 1];
        const int w = ex - sx, hgt = ey - sy;
        if (w > 0 && hgt > 0 && off >= 0 && off + n <= a.lin_len) {
            for (int k = threadIdx.x; k < w * hgt; k += blockDim.x) {
                const int dy = k / w, dx = k - dy * w;
                const int pi = psy + dy, pj = psx + dx;        // profile row / column
                if (pi < 0 || pi >= n || pj < 0 || pj >= n) continue;
                const float xi = a.lin[off + pi], yj = a.lin[off + pj];
                const float d = sqrtf(__fadd_rn(__fmul_rn(xi, xi), __fmul_rn(yj, yj)));     // IEEE sqrt (bn_device_math.h sqrt_cr)
                const float p = d <= r ? __fmul_rn(nt, __fsub_rn(r, d)) : 0.0f;
                if (p != 0.0f) {
                    float *cell = h + (size_t)(sy + dy) * N + (sx + dx);
                    *cell = __fadd_rn(*cell, p);
                }
            }
        }
        __syncthreads();
        block_min_shift(h, cells, red);
    }
}

__global__ __launch_bounds__(kReduceThreads) void terrain_minshift_kernel(TerrainArgs a)
{
    __shared__ float red[kReduceThreads];
    block_min_shift(a.hp + (size_t)blockIdx.x * a.N * a.N, a.N * a.N, red);
}

// One entry of the fBm grid in its final state.  Loop 1 (y, x <= h = N/2) writes A(y, x) = rad e^{i phi} at (y, x) and, for
// x, y > 0, conj(A) at (N-y, N-x); the three edge / corner entries are then made real; loop 2 (1 <= y, x <= h-1) writes B(y, x)
// at (y, N-x) and conj(B) at (N-y, x).  The write sets of loop 2 and loop 1 are disjoint and loop 1's direct and mirrored sets
// meet only at (h, h) for even N (same iteration, mirror last, then made real), so checking the writers from the last to the
// first gives the last writer of every cell.  Cells no loop writes stay 0 (odd N leaves some).
__device__ double2 spectrum_entry(const TerrainArgs &a, const float *ph, int r, int c)
{
    const int N = a.N, hN = N / 2;
    int y, x, idx;
    bool conj = false, real_only = false;
    if (r >= N - hN + 1 && r <= N - 1 && c >= 1 && c <= hN - 1) {            // loop 2, mirror
        y = N - r; x = c; conj = true; idx = (hN + 1) * (hN + 1) + (y - 1) * (hN - 1) + (x - 1);
    } else if (r >= 1 && r <= hN - 1 && c >= N - hN + 1 && c <= N - 1) {     // loop 2, direct
        y = r; x = N - c; idx = (hN + 1) * (hN + 1) + (y - 1) * (hN - 1) + (x - 1);
    } else if ((r == hN && c == 0) || (r == 0 && c == hN) || (r == hN && c == hN)) {
        y = r; x = c; real_only = true; idx = y * (hN + 1) + x;
    } else if (r >= N - hN && c >= N - hN && r <= N - 1 && c <= N - 1) {     // loop 1, mirror
        y = N - r; x = N - c; conj = true; idx = y * (hN + 1) + x;
    } else if (r <= hN && c <= hN) {                                          // loop 1, direct
        y = r; x = c; idx = y * (hN + 1) + x;
    } else {
        return make_double2(0.0, 0.0);
    }
    if (x == 0 && y == 0) return make_double2(0.0, 0.0);                     // rad = 0 at the origin
    if (idx < 0 || idx >= a.nph) return make_double2(0.0, 0.0);
    const float phi = __fmul_rn(6.2831855f, ph[idx]);                          // 2 * torch.pi * rand(1), in float32
    const double rad = pow((double)(x * x + y * y), a.expo) * a.scale;
    double s, co;
    sincos((double)phi, &s, &co);
    const double im = real_only ? 0.0 : (conj ? -s : s);
    return make_double2(rad * co, rad * im);
}

__global__ void terrain_spectrum_kernel(TerrainArgs a)
{
    const size_t cells = (size_t)a.N * a.N;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cells * a.B) return;
    const int b = (int)(i / cells);
    const int rem = (int)(i - (size_t)b * cells);
    const int r = rem / a.N, c = rem - r * a.N;
    const double2 v = spectrum_entry(a, a.phases + (size_t)b * a.nph, r, c);
    a.S[i] = make_float2((float)v.x, (float)v.y);
}

// T[b, k, x] = sum_l S[b, k, l] tw[(l x) mod N]; block (kTile, kTile) = (x, k), grid (x tiles, k tiles, B)
__global__ __launch_bounds__(kTile * kTile) void terrain_dft_rows_kernel(TerrainArgs a)
{
    __shared__ double2 tw[kMaxN];
    __shared__ double2 st[kTile][kTile + 1];
    const int N = a.N, b = blockIdx.z;
    const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * kTile + tx;
    for (int m = tid; m < N; m += kTile * kTile) tw[m] = a.tw[m];
    const int x = blockIdx.x * kTile + tx, k = blockIdx.y * kTile + ty;
    const float2 *S = a.S + (size_t)b * N * N;
    double re = 0.0, im = 0.0;
    int idx = 0;                                                 // (l x) mod N, advanced by x per l
    const int xs = x < N ? x : 0;
    for (int l0 = 0; l0 < N; l0 += kTile) {
        __syncthreads();
        {
            const int kk = blockIdx.y * kTile + ty, ll = l0 + tx;
            float2 v = make_float2(0.0f, 0.0f);
            if (kk < N && ll < N) v = S[(size_t)kk * N + ll];
            st[ty][tx] = make_double2(v.x, v.y);
        }
        __syncthreads();
        const int lmax = min(kTile, N - l0);
        for (int j = 0; j < lmax; ++j) {
            const double2 s = st[ty][j];
            const double2 w = tw[idx];
            re = fma(s.x, w.x, re); re = fma(-s.y, w.y, re);
            im = fma(s.x, w.y, im); im = fma(s.y, w.x, im);
            idx += xs;
            if (idx >= N) idx -= N;
        }
    }
    if (x < N && k < N) a.T[((size_t)b * N + k) * N + x] = make_double2(re, im);
}

// out[b, y, x] = Re sum_k tw[(k y) mod N] T[b, k, x] / N^2 -> float32, then / f32((res 1e3)^2), * f32(1e-3), added to hp
__global__ __launch_bounds__(kTile * kTile) void terrain_dft_cols_kernel(TerrainArgs a)
{
    __shared__ double2 tw[kMaxN];
    __shared__ double2 tt[kTile][kTile + 1];
    const int N = a.N, b = blockIdx.z;
    const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * kTile + tx;
    for (int m = tid; m < N; m += kTile * kTile) tw[m] = a.tw[m];
    const int x = blockIdx.x * kTile + tx, y = blockIdx.y * kTile + ty;
    const double2 *T = a.T + (size_t)b * N * N;
    double re = 0.0;
    int idx = 0;
    const int ys = y < N ? y : 0;
    for (int k0 = 0; k0 < N; k0 += kTile) {
        __syncthreads();
        {
            const int kk = k0 + ty, xx = blockIdx.x * kTile + tx;
            tt[ty][tx] = (kk < N && xx < N) ? T[(size_t)kk * N + xx] : make_double2(0.0, 0.0);
        }
        __syncthreads();
        const int kmax = min(kTile, N - k0);
        for (int j = 0; j < kmax; ++j) {
            const double2 t = tt[j][tx];
            const double2 w = tw[idx];
            re = fma(t.x, w.x, re); re = fma(-t.y, w.y, re);
            idx += ys;
            if (idx >= N) idx -= N;
        }
    }
    if (x < N && y < N) {
        float s = (float)(re / ((double)N * (double)N));
        s = __fdiv_rn(s, a.c_div);
        s = __fmul_rn(s, a.c_milli);
        float *cell = a.hp + ((size_t)b * N + y) * N + x;
        *cell = __fadd_rn(*cell, s);
    }
}

// crop + Horn slopes + latent slip model for every output cell
__global__ void terrain_surface_kernel(TerrainArgs a)
{
    const int G = a.G, N = a.N;
    const size_t cells = (size_t)G * G;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cells * a.B) return;
    const int b = (int)(i / cells);
    const int rem = (int)(i - (size_t)b * cells);
    const int r = rem / G, c = rem - r * G;
    const float *h = a.hp + (size_t)b * N * N + (size_t)(r + 1) * N + (c + 1);   // padded (r+1, c+1); neighbours are inside
    const double h00 = h[-N - 1], h01 = h[-N], h02 = h[-N + 1];
    const double h10 = h[-1], h12 = h[1];
    const double h20 = h[N - 1], h21 = h[N], h22 = h[N + 1];
    // Sobel cross-correlation (conv2d): x = [-1 0 1; -2 0 2; -1 0 1], y = [-1 -2 -1; 0 0 0; 1 2 1]
    const double gx = ((h02 - h00) + 2.0 * (h12 - h10) + (h22 - h20)) * a.inv_8res;
    const double gy = ((h20 - h00) + 2.0 * (h21 - h01) + (h22 - h02)) * a.inv_8res;
    const float phi = (float)(atan(sqrt(gx * gx + gy * gy)) * (180.0 / M_PI));
    a.heights[i] = h[0];
    a.slopes[i] = phi;
    const int cls = a.classes[i];
    float m = INFINITY, sd = INFINITY;                            // set_traversability starts from inf
    if (cls >= 0 && cls < a.nclass) {
        const float *p = a.cparams + (size_t)cls * kClassParams;
        if (p[0] != 0.0f) {
            const float aphi = fabsf(phi);
            const float base = __fmul_rn(p[1], powf(aphi, p[2]));
            const float s = phi >= 0.0f ? __fadd_rn(base, p[3]) : __fadd_rn(-base, p[3]);
            m = fminf(fmaxf(s, 0.0f), 1.0f);
            sd = __fadd_rn(p[4], __fmul_rn(p[5], aphi));
        }
    }
    a.mean[i] = m;
    a.stddev[i] = sd;
}

// the test hook's copy of one instance's spectrum
__global__ void terrain_spectrum_one_kernel(TerrainArgs a, int inst, float2 *out)
{
    const int cells = a.N * a.N;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cells) return;
    const int r = i / a.N, c = i - r * a.N;
    const double2 v = spectrum_entry(a, a.phases + (size_t)inst * a.nph, r, c);
    out[i] = make_float2((float)v.x, (float)v.y);
}

// ---- terrain classes and shaded colours (TerrainColoring.set_terrain_class_coloring, terrain_properties.py:364-523) ----
struct ColorArgs {
    float *noise;              // (B, G, G) raw noise field: uploaded, or written by terrain_noise_kernel
    int32_t *classes;          // (B, G, G): written by terrain_classes_kernel, read by terrain_color_kernel
    const float *heights;      // (B, G, G) cropped heights
    float *colors;             // (B, 3, G, G)
    const float *thr;          // (B, C) float32 cumsum(occupancy) * 100, from the host's torch
    const int32_t *start;      // (B) first class with occupancy > 0
    const float *table;        // (C, 3) colour table
    const float *light;        // (B, 3) light vectors
    const uint64_t *seeds;     // (B) keys of the library's own noise
    int32_t *counts;           // (B, 2): cells with class -1, cells with class >= nmodels
    int G, B, C, nmodels;
    float feature, ambient;
};

// The library's own 2-D gradient noise: float32, every operation rounded on its own (no FMA anywhere), in this
// order.  u = f32(x) / f, v = f32(y) / f (IEEE division); i = floor(u), j = floor(v); p = u - i, q = v - j.  The gradient of
// lattice point (a, b) is row (w & 7) of kGrad, w the first word of Philox4x32-10 on the counter (a, b, 'TNOI', 0) under the
// key (lo(seed), hi(seed)).  d00 = gx p + gy q and likewise d10 (p - 1, q), d01 (p, q - 1), d11 (p - 1, q - 1) from the
// gradients of (i, j), (i+1, j), (i, j+1), (i+1, j+1); fade(t) = ((t t) t) ((t (t 6 - 15)) + 10);
// n = l0 + fade(q) (l1 - l0), l0 = d00 + fade(p) (d10 - d00), l1 = d01 + fade(p) (d11 - d01).  Zero at lattice points.
constexpr uint32_t kNoiseWord = 0x544E4F49u;                                  // 'TNOI'
constexpr float kDiag = 0.70710677f;
__constant__ float kGrad[8][2] = {{1.0f, 0.0f}, {-1.0f, 0.0f}, {0.0f, 1.0f}, {0.0f, -1.0f},
                                  {kDiag, kDiag}, {-kDiag, kDiag}, {kDiag, -kDiag}, {-kDiag, -kDiag}};

__device__ __forceinline__ float noise_fade(float t)
{
    const float a = __fsub_rn(__fmul_rn(t, 6.0f), 15.0f);
    const float b = __fadd_rn(__fmul_rn(t, a), 10.0f);
    return __fmul_rn(__fmul_rn(__fmul_rn(t, t), t), b);
}

__device__ __forceinline__ float noise_corner(uint64_t seed, int a, int b, float p, float q)
{
    const u32x4 w = philox4x32_10(u32x4{(uint32_t)a, (uint32_t)b, kNoiseWord, 0u}, (uint32_t)seed, (uint32_t)(seed >> 32));
    const int g = (int)(w.x & 7u);
    return __fadd_rn(__fmul_rn(kGrad[g][0], p), __fmul_rn(kGrad[g][1], q));
}

__global__ void terrain_noise_kernel(ColorArgs a)
{
    const size_t cells = (size_t)a.G * a.G;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cells * a.B) return;
    const int b = (int)(i / cells);
    const int rem = (int)(i - (size_t)b * cells);
    const int y = rem / a.G, x = rem - y * a.G;
    const uint64_t seed = a.seeds[b];
    const float u = __fdiv_rn((float)x, a.feature), v = __fdiv_rn((float)y, a.feature);
    const float fi = floorf(u), fj = floorf(v);
    const int ci = (int)fi, cj = (int)fj;
    const float p = __fsub_rn(u, fi), q = __fsub_rn(v, fj);
    const float p1 = __fsub_rn(p, 1.0f), q1 = __fsub_rn(q, 1.0f);
    const float d00 = noise_corner(seed, ci, cj, p, q), d10 = noise_corner(seed, ci + 1, cj, p1, q);
    const float d01 = noise_corner(seed, ci, cj + 1, p, q1), d11 = noise_corner(seed, ci + 1, cj + 1, p1, q1);
    const float wp = noise_fade(p), wq = noise_fade(q);
    const float l0 = __fadd_rn(d00, __fmul_rn(wp, __fsub_rn(d10, d00)));
    const float l1 = __fadd_rn(d01, __fmul_rn(wp, __fsub_rn(d11, d01)));
    a.noise[i] = __fadd_rn(l0, __fmul_rn(wq, __fsub_rn(l1, l0)));
}

// generate_multi_terrain :421-443 for instance blockIdx.x: the field's min and max, nd = (n - min) / (max - min) * 100 in that
// order, class = the smallest i >= start with nd <= thr[i], else -1 (every comparison is false on the NaN field of max == min).
// With thr non-decreasing (a cumsum of non-negative ratios) that is the reference's chain of masks.
constexpr int kMaxColorClasses = 64;

__global__ __launch_bounds__(kReduceThreads) void terrain_classes_kernel(ColorArgs a)
{
    __shared__ float rmin[kReduceThreads], rmax[kReduceThreads];
    __shared__ float thr[kMaxColorClasses];
    __shared__ int cnt[2];
    const int b = blockIdx.x, cells = a.G * a.G, C = min(a.C, kMaxColorClasses);
    const float *n = a.noise + (size_t)b * cells;
    int32_t *cls = a.classes + (size_t)b * cells;
    if ((int)threadIdx.x < C) thr[threadIdx.x] = a.thr[(size_t)b * a.C + threadIdx.x];
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
    float mn = INFINITY, mx = -INFINITY;
    for (int i = threadIdx.x; i < cells; i += blockDim.x) { const float v = n[i]; mn = fminf(mn, v); mx = fmaxf(mx, v); }
    rmin[threadIdx.x] = mn; rmax[threadIdx.x] = mx;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            rmin[threadIdx.x] = fminf(rmin[threadIdx.x], rmin[threadIdx.x + s]);
            rmax[threadIdx.x] = fmaxf(rmax[threadIdx.x], rmax[threadIdx.x + s]);
        }
        __syncthreads();
    }
    mn = rmin[0]; mx = rmax[0];
    const float range = __fsub_rn(mx, mn);
    const int start = min(max(a.start[b], 0), C);
    int unassigned = 0, beyond = 0;
    for (int i = threadIdx.x; i < cells; i += blockDim.x) {
        const float nd = __fmul_rn(__fdiv_rn(__fsub_rn(n[i], mn), range), 100.0f);
        int c = -1;
        for (int k = start; k < C; ++k)
            if (nd <= thr[k]) { c = k; break; }
        cls[i] = c;
        unassigned += c < 0;
        beyond += c >= a.nmodels;
    }
    if (unassigned) atomicAdd(&cnt[0], unassigned);
    if (beyond) atomicAdd(&cnt[1], beyond);
    __syncthreads();
    if (threadIdx.x < 2) a.counts[b * 2 + threadIdx.x] = cnt[threadIdx.x];
}

// create_color_map :462-470 + create_shading :491-523, one thread per cell.  dx, dy one-sided at the borders and halved in the
// interior, norm = (nx, ny, 1) / sqrt((nx^2 + ny^2) + 1), shade = (Lx nx + Ly ny) + Lz nz, colour = clamp(shade c + ambient c, 0, 1)
// with c the class's table row: a class below 0 takes row 0 and one above C - 1 row C - 1, as the colour map's under / over entries.
__global__ __launch_bounds__(256) void terrain_color_kernel(ColorArgs a)
{
    __shared__ float tab[kMaxColorClasses * 3];
    const int G = a.G, C = min(a.C, kMaxColorClasses);
    for (int k = threadIdx.x; k < C * 3; k += blockDim.x) tab[k] = a.table[k];
    __syncthreads();
    const size_t cells = (size_t)G * G;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cells * a.B) return;
    const int b = (int)(i / cells);
    const int rem = (int)(i - (size_t)b * cells);
    const int r = rem / G, c = rem - r * G;
    const float *h = a.heights + (size_t)b * cells + rem;
    const float h0 = h[0];
    float nx = 0.0f, ny = 0.0f;
    if (c < G - 1) nx = __fadd_rn(nx, __fsub_rn(h0, h[1]));
    if (c > 0) nx = __fadd_rn(nx, __fsub_rn(h[-1], h0));
    if (c > 0 && c < G - 1) nx = __fdiv_rn(nx, 2.0f);
    if (r < G - 1) ny = __fadd_rn(ny, __fsub_rn(h0, h[G]));
    if (r > 0) ny = __fadd_rn(ny, __fsub_rn(h[-G], h0));
    if (r > 0 && r < G - 1) ny = __fdiv_rn(ny, 2.0f);
    const float len = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(nx, nx), __fmul_rn(ny, ny)), 1.0f));
    const float ux = __fdiv_rn(nx, len), uy = __fdiv_rn(ny, len), uz = __fdiv_rn(1.0f, len);
    const float *L = a.light + (size_t)b * 3;
    const float shade = __fadd_rn(__fadd_rn(__fmul_rn(L[0], ux), __fmul_rn(L[1], uy)), __fmul_rn(L[2], uz));
    const int cls = min(max(a.classes[i], 0), C - 1);
    float *out = a.colors + (size_t)b * 3 * cells + rem;
    for (int k = 0; k < 3; ++k) {
        const float col = tab[cls * 3 + k];
        const float v = __fadd_rn(__fmul_rn(shade, col), __fmul_rn(a.ambient, col));
        out[(size_t)k * cells] = fminf(fmaxf(v, 0.0f), 1.0f);
    }
}

// ---- the random draws on the device (DESIGN.md 4.5 "The draws on the device") ----
// What terrain.replay_draws makes on torch's CPU generator, for instance blockIdx.x from seeds[blockIdx.x]: MT19937 seeded with
// the seed's low 32 bits, one float32 uniform f32(r & 0xFFFFFF) 2^-24 per 32-bit output r; the crater rejection loop (three
// uniforms per attempt, a fourth for an accepted one), each accepted crater's table entry, then the nph fBm phases and, for
// the colouring, the two uniforms of the light source.  The generator is mt19937.h's (two 624-word blocks in LDS).
constexpr int kDrawThreads = 256;          // >= 227: each of the twist's parallel segments is one word per thread
constexpr int kMaxDrawCraters = 64;        // placed craters' centres and radii live in LDS
constexpr int kMaxAttempts = 1000;         // terrain_properties.py:124
constexpr int kDrawRecord = 4;             // attempts, gave_up, status (0, or 1 + the first crater that does not fit), craters placed

struct DrawArgs {
    const uint64_t *seeds;     // (B)
    float *phases;             // (B, nph)
    int32_t *cr_count, *cr_int;
    float *cr_val, *lin;       // lin: (B, maxc, stride), slot (b, c) at offset (b maxc + c) stride
    float *light;              // (B, 3), with_light only
    int32_t *rec;              // (B, kDrawRecord)
    float *centers;            // (B, maxc, 2)
    double *angles;            // (B, maxc) degrees
    float *light_u;            // (B, 2)
    int G, N, nph, maxc, stride, want, fractal, with_light;
    float span, org, res;      // f32((N - 1) res - x0), f32(x0), f32(res)
    float rspan, rmin, margin; // f32(max_radius - min_radius), f32(min_radius), f32(crater_margin)
    float lspan, llo;          // f32(upper_threshold - lower_threshold), f32(lower_threshold)
    double aspan, amin;        // max_angle - min_angle, min_angle
};

// One attempt of the crater loop from its three state words: the centre and the radius, and whether it overlaps a placed crater
// (check_circle_overlap: norm(p - c) < (r_p + r) + margin for any p).
__device__ __forceinline__ bool crater_attempt(const DrawArgs &a, const uint32_t *w, const float *px, const float *py, const float *pr,
                                               int placed, float &cx, float &cy, float &r)
{
    cx = __fadd_rn(__fmul_rn(mt_uniform(w[0]), a.span), a.org);
    cy = __fadd_rn(__fmul_rn(mt_uniform(w[1]), a.span), a.org);
    r = __fadd_rn(__fmul_rn(mt_uniform(w[2]), a.rspan), a.rmin);
    bool overlap = false;
    for (int p = 0; p < placed; ++p) {
        const float dx = __fsub_rn(px[p], cx), dy = __fsub_rn(py[p], cy);
        const float dist = sqrtf(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));
        overlap = overlap || dist < __fadd_rn(__fadd_rn(pr[p], r), a.margin);
    }
    return overlap;
}

__global__ __launch_bounds__(kDrawThreads) void terrain_draws_kernel(DrawArgs a)
{
    __shared__ uint32_t mt[2][kMtN];
    __shared__ float px[kMaxDrawCraters], py[kMaxDrawCraters], pr[kMaxDrawCraters];
    __shared__ int first;
    const int b = blockIdx.x, t = threadIdx.x, G = a.G, N = a.N;
    if (t == 0) mt_seed(mt[0], (uint32_t)a.seeds[b]);                        // init_genrand: a dependent chain
    __syncthreads();
    MtStream s{mt, 0, kMtN};                                                 // the first draw twists first
    const int want = min(a.want, min(a.maxc, kMaxDrawCraters));
    int placed = 0, attempts = 0, gave_up = 0, status = 0;
    // A rejected attempt takes exactly three uniforms, so until one is accepted attempt j of a run reads words pos + 3 j ...
    // pos + 3 j + 2: the threads try the attempts that fit the rest of this block of the stream at once, against the same placed
    // craters, and the first one that does not overlap is the accepted one.  An attempt that straddles two blocks is tried alone.
    while (placed < want) {
        const int room = (kMtN - s.pos) / 3;
        float cx = 0.0f, cy = 0.0f, r = 0.0f;
        bool accepted;
        if (room > 0) {
            const int w = min(min(room, kMaxAttempts + 1 - attempts), kDrawThreads);
            const uint32_t *m = s.mt[s.cur] + s.pos;
            if (t == 0) first = w;
            __syncthreads();
            if (t < w && !crater_attempt(a, m + 3 * t, px, py, pr, placed, cx, cy, r)) atomicMin(&first, t);
            __syncthreads();
            const int k = __builtin_amdgcn_readfirstlane(first);
            __syncthreads();                                                 // everyone has read `first` before it is set again
            accepted = k < w;
            const int used = accepted ? k + 1 : w;
            if (accepted) crater_attempt(a, m + 3 * k, px, py, pr, placed, cx, cy, r);
            s.pos += 3 * used;
            attempts += used;
        } else {
            uint32_t u[3];
            for (int i = 0; i < 3; ++i) u[i] = mt_word(s);
            accepted = __builtin_amdgcn_readfirstlane((int)!crater_attempt(a, u, px, py, pr, placed, cx, cy, r)) != 0;
            ++attempts;
        }
        if (accepted) {
            const double angle = (double)mt_next(s) * a.aspan + a.amin;      // no FMA (-ffp-contract=off)
            // _crater_plan: profile size, centre cell, slice bounds
            const float two_r = __fadd_rn(r, r);
            const int n = (int)ceilf(__fdiv_rn(two_r, a.res));
            const int ccx = min(max((int)floorf(__fdiv_rn(__fsub_rn(cx, a.org), a.res)), 0), G - 1);
            const int ccy = min(max((int)floorf(__fdiv_rn(__fsub_rn(cy, a.org), a.res)), 0), G - 1);
            const int half = n / 2;
            const int sx = max(ccx - half, 0), sy = max(ccy - half, 0), ex = min(ccx + half, N), ey = min(ccy + half, N);
            const int psx = max(half - ccx, 0), psy = max(half - ccy, 0);
            const bool fits = n >= 1 && n <= a.stride && psx + (ex - sx) <= n && psy + (ey - sy) <= n;
            if (!fits && status == 0) status = placed + 1;
            const size_t slot = (size_t)b * a.maxc + placed;
            const int off = (int)(slot * a.stride);
            // torch's scalar linspace(-r, r, n)
            const float step = n > 1 ? __fdiv_rn(two_r, (float)(n - 1)) : 0.0f;
            for (int i = t; i < n && i < a.stride; i += kDrawThreads)
                a.lin[off + i] = i < half ? __fadd_rn(-r, __fmul_rn(step, (float)i)) : __fsub_rn(r, __fmul_rn(step, (float)(n - 1 - i)));
            if (t == 0) {
                px[placed] = cx; py[placed] = cy; pr[placed] = r;
                int32_t *ci = a.cr_int + slot * 8;
                ci[0] = sx; ci[1] = sy; ci[2] = ex; ci[3] = ey; ci[4] = psx; ci[5] = psy; ci[6] = n;
                ci[7] = fits ? off : -1;                                     // the crater kernel carves offsets >= 0 only
                const float rad = __fmul_rn((float)angle, (float)(M_PI / 180.0));          // deg2rad in float32
                a.cr_val[slot * 2] = r;
                a.cr_val[slot * 2 + 1] = (float)(-tan((double)rad));
                a.centers[slot * 2] = cx; a.centers[slot * 2 + 1] = cy;
                a.angles[slot] = angle;
            }
            __syncthreads();
            ++placed;
        }
        if (attempts > kMaxAttempts) { gave_up = 1; break; }                 // count > 1000 after the attempt, accepted or not
    }
    if (a.fractal) {                                                         // generate_fractal_surface's uniforms, a block at a time
        float *ph = a.phases + (size_t)b * a.nph;
        for (int k = 0; k < a.nph;) {
            if (s.pos == kMtN) mt_refill(s);
            const int m = min(a.nph - k, kMtN - s.pos);
            for (int i = t; i < m; i += kDrawThreads) ph[k + i] = mt_uniform(s.mt[s.cur][s.pos + i]);
            k += m;
            s.pos += m;
        }
    }
    float ua = 0.0f, uz = 0.0f;
    if (a.with_light) {                                                      // create_shading :511-517
        ua = mt_next(s);
        uz = mt_next(s);
    }
    if (t == 0) {
        a.cr_count[b] = placed;
        int32_t *rec = a.rec + (size_t)b * kDrawRecord;
        rec[0] = attempts; rec[1] = gave_up; rec[2] = status; rec[3] = placed;
        a.light_u[b * 2] = ua; a.light_u[b * 2 + 1] = uz;
        if (a.with_light) {
            const float ang = __fmul_rn(ua, (float)(2.0 * M_PI));
            const float z = __fadd_rn(__fmul_rn(uz, a.lspan), a.llo);
            const float rad = sqrtf(__fsub_rn(1.0f, __fmul_rn(z, z)));
            double sn, cs;
            sincos((double)ang, &sn, &cs);
            a.light[b * 3] = __fmul_rn(rad, (float)cs);
            a.light[b * 3 + 1] = __fmul_rn(rad, (float)sn);
            a.light[b * 3 + 2] = z;
        }
    }
}

thread_local std::string g_terrain_error;

}  // namespace
}  // namespace bn

struct bn_terrain {
    int device = 0, G = 0, N = 0, B = 0, nph = 0;
    double resolution = 0.5, roughness = 0.75, gain = 10.0;
    bool fractal = true, have_geometry = false, have_draws = false, have_slip = false, generated = false;
    float *hp = nullptr, *heights = nullptr, *slopes = nullptr, *mean = nullptr, *stddev = nullptr, *phases = nullptr;
    float2 *S = nullptr;
    double2 *T = nullptr, *tw = nullptr;
    int32_t *classes = nullptr, *cr_count = nullptr, *cr_int = nullptr;
    float *cr_val = nullptr, *lin = nullptr, *cparams = nullptr;
    int maxc = 0, lin_len = 0, nclass = -1;  // what cr_int / cr_val, lin and cparams are sized for (nothing yet)
    hipEvent_t ev_done = nullptr;
    // colouring (allocated by the first bn_terrain_set_coloring / bn_terrain_colorize)
    bool coloring = false, own_noise = false, colored = false, ev_recorded = false;
    int ncolor = 0, nmodels = 0;
    float feature = 20.0f, ambient = 0.1f;
    float *noise = nullptr, *colors = nullptr, *thr = nullptr, *ctable = nullptr, *light = nullptr, *cz_heights = nullptr;
    int32_t *cstart = nullptr, *counts = nullptr, *cz_classes = nullptr;
    uint64_t *cseeds = nullptr;
    // the draws on the device (bn_terrain_set_draw_params / bn_terrain_draw_async)
    bool have_draw_params = false, drawn = false, dr_crater = true, dr_light = false;
    int dr_num = 0, dr_slots = 0;            // craters asked for; slots the record buffers were sized for
    double dr_margin = 5.0, dr_amin = 10.0, dr_amax = 20.0, dr_rmin = 5.0, dr_rmax = 10.0, dr_llo = 0.8, dr_lhi = 1.0;
    uint64_t *dseeds = nullptr, *dseeds_pinned = nullptr;      // pinned staging: the seeds reach the device on the caller's stream
    int32_t *drec = nullptr;
    float *dcenters = nullptr, *dlight_u = nullptr;
    double *dangles = nullptr;
    // the table of all of the above (bn_host.h): `bufs` from bn_terrain_create on, the groups from their first use
    bn::DeviceBuffers bufs, color, draw, stage;
};

namespace {

int terrain_fail(int code, const std::string &msg)
{
    bn::g_terrain_error = msg;
    return code;
}

#define TERRAIN_HIP(expr) BN_HIP_AS(terrain_fail, expr, #expr)

#define TERRAIN_ON_DEVICE(h) BN_ON_DEVICE(terrain_fail, (h)->device)

int wait_done(bn_terrain_t *h)
{
    if (h->generated || h->ev_recorded) TERRAIN_HIP(hipEventSynchronize(h->ev_done));
    return BN_OK;
}

bn::TerrainArgs make_args(bn_terrain_t *h)
{
    const double res = h->resolution, H = h->roughness;
    bn::TerrainArgs a{};
    a.hp = h->hp; a.S = h->S; a.T = h->T; a.tw = h->tw; a.phases = h->phases;
    a.cr_count = h->cr_count; a.cr_int = h->cr_int; a.cr_val = h->cr_val; a.lin = h->lin;
    a.classes = h->classes; a.cparams = h->cparams;
    a.heights = h->heights; a.slopes = h->slopes; a.mean = h->mean; a.stddev = h->stddev;
    a.G = h->G; a.N = h->N; a.B = h->B; a.nph = h->nph; a.maxc = h->maxc; a.lin_len = h->lin_len; a.nclass = h->nclass;
    a.expo = -((H + 1.0) / 2.0);
    a.scale = (double)(float)(std::fabs(h->gain) * std::pow(h->N * res * 1e3, H + 1.0 + 0.5));
    a.c_div = (float)std::pow(res * 1e3, 2.0);
    a.c_milli = (float)1e-3;
    a.inv_8res = 1.0 / (8.0 * res);
    return a;
}

bn::ColorArgs make_color_args(bn_terrain_t *h)
{
    bn::ColorArgs a{};
    a.noise = h->noise; a.classes = h->classes; a.heights = h->heights; a.colors = h->colors; a.thr = h->thr; a.start = h->cstart;
    a.table = h->ctable; a.light = h->light; a.seeds = h->cseeds; a.counts = h->counts;
    a.G = h->G; a.B = h->B; a.C = h->ncolor; a.nmodels = h->nmodels; a.feature = h->feature; a.ambient = h->ambient;
    return a;
}

// the colouring buffers whose size depends on G and B alone (the first use allocates them), and the (C, 3) table
int ensure_color_buffers(bn_terrain_t *h, int C)
{
    int rc = h->color.ensure(terrain_fail);
    if (rc) return rc;
    if (C != h->ncolor) {
        h->ncolor = 0;
        if ((rc = h->color.resize(&h->thr, (size_t)h->B * C * 4, terrain_fail)) || (rc = h->color.resize(&h->ctable, (size_t)C * 12, terrain_fail)))
            return rc;
        h->ncolor = C;
    }
    return BN_OK;
}

// The crater tables for `slots` craters an instance, and the profile table for `len` values (it only grows; lin_len is the
// length in use).  Both size fields are void while their buffers are being replaced: a failure leaves them asking for the
// replacement again.
int resize_craters(bn_terrain_t *h, int slots)
{
    int rc = BN_OK;
    h->maxc = 0;
    if ((rc = h->bufs.resize(&h->cr_int, (size_t)h->B * slots * 32, terrain_fail)) || (rc = h->bufs.resize(&h->cr_val, (size_t)h->B * slots * 8, terrain_fail)))
        return rc;
    h->maxc = slots;
    return BN_OK;
}

int fit_lin(bn_terrain_t *h, int64_t len)
{
    if (len > h->lin_len) {
        h->lin_len = 0;
        if (int rc = h->bufs.resize(&h->lin, (size_t)len * 4, terrain_fail)) return rc;
    }
    h->lin_len = (int)len;
    return BN_OK;
}

// profile points a crater slot of the device draws holds: ceil(f32(2 r) / f32(res)) for the largest radius, and two to spare
int64_t draw_stride(const bn_terrain_t *h)
{
    const double rmax = std::max(h->dr_rmin, h->dr_rmax);
    return (int64_t)std::ceil(2.0 * rmax / h->resolution) + 2;
}

// Size the crater tables, the profile slots and the per-instance records for the draw parameters as they stand (a host
// bn_terrain_set_draws in between may have resized the tables).  Waits for the handle's work before it frees anything.
int ensure_draw_buffers(bn_terrain_t *h)
{
    const int slots = std::max(h->dr_crater ? h->dr_num : 0, 1);
    const int64_t need = (int64_t)h->B * slots * draw_stride(h);
    if (need > ((int64_t)1 << 30)) return terrain_fail(BN_ERR_INVALID, "the crater profiles (B x num_craters x 2 max_radius / resolution) must fit 2^30 values");
    int rc = BN_OK;
    if (slots != h->maxc || slots != h->dr_slots || need > h->lin_len || !h->draw.live) {
        if ((rc = wait_done(h))) return rc;
    }
    if ((rc = h->draw.ensure(terrain_fail))) return rc;
    if (slots != h->maxc && (rc = resize_craters(h, slots))) return rc;
    if (slots != h->dr_slots) {
        h->dr_slots = 0;
        if ((rc = h->draw.resize(&h->dcenters, (size_t)h->B * slots * 8, terrain_fail)) || (rc = h->draw.resize(&h->dangles, (size_t)h->B * slots * 8, terrain_fail)))
            return rc;
        h->dr_slots = slots;
    }
    return fit_lin(h, need);
}

// What bn_terrain_create builds on the device: every buffer of the handle entered in its table, the ones every generation needs
// allocated, and the DFT's twiddle factors.
int terrain_init(bn_terrain_t *h)
{
    const size_t pc = (size_t)h->N * h->N * h->B, oc = (size_t)h->G * h->G * h->B, sB = (size_t)h->B;
    std::vector<double2> tw(h->N);
    for (int m = 0; m < h->N; ++m) {
        const double t = 2.0 * M_PI * (double)m / (double)h->N;
        tw[m] = make_double2(std::cos(t), std::sin(t));
    }
    bn::DeviceBuffers &m = h->bufs, &c = h->color, &d = h->draw, &z = h->stage;
    m.add(&h->hp, pc * 4); m.add(&h->S, pc * 8); m.add(&h->T, pc * 16); m.add(&h->tw, (size_t)h->N * 16);
    m.add(&h->heights, oc * 4); m.add(&h->slopes, oc * 4); m.add(&h->mean, oc * 4); m.add(&h->stddev, oc * 4);
    m.add(&h->classes, oc * 4); m.add(&h->phases, (size_t)h->nph * sB * 4); m.add(&h->cr_count, sB * 4);
    // sized by the draws and the slip models as they are set (maxc, lin_len and nclass say for what)
    m.add_later(&h->cr_int); m.add_later(&h->cr_val); m.add_later(&h->lin); m.add_later(&h->cparams);
    m.add_event(&h->ev_done);
    // the colouring: sized by G and B alone, and the two tables that follow the number of classes (ncolor)
    c.add(&h->noise, oc * 4); c.add(&h->colors, oc * 12); c.add(&h->light, sB * 12); c.add(&h->cstart, sB * 4);
    c.add(&h->counts, sB * 8); c.add(&h->cseeds, sB * 8); c.add_later(&h->thr); c.add_later(&h->ctable);
    // the device draws: the records, and the two tables that follow the crater slots (dr_slots)
    d.add(&h->dseeds, sB * 8); d.add_pinned(&h->dseeds_pinned, sB * 8); d.add(&h->drec, sB * bn::kDrawRecord * 4);
    d.add(&h->dlight_u, sB * 8); d.add_later(&h->dcenters); d.add_later(&h->dangles);
    // bn_terrain_colorize's copies of the caller's maps
    z.add(&h->cz_heights, oc * 4); z.add(&h->cz_classes, oc * 4);
    if (int rc = m.alloc_all(terrain_fail)) return rc;
    TERRAIN_HIP(hipMemcpy(h->tw, tw.data(), (size_t)h->N * 16, hipMemcpyHostToDevice));
    return BN_OK;
}

}  // namespace

extern "C" {

const char *bn_terrain_last_error(void) { return bn::g_terrain_error.c_str(); }

int bn_terrain_create(int32_t device_id, int32_t G, int32_t B, bn_terrain_t **out)
{
    if (!out) return terrain_fail(BN_ERR_INVALID, "null handle pointer");
    *out = nullptr;
    if (G < 2 || G + 2 > bn::kMaxN || B < 1 || (int64_t)(G + 2) * (G + 2) * B > ((int64_t)1 << 31))
        return terrain_fail(BN_ERR_INVALID, "G must be in [2, 1024], B >= 1, and B (G+2)^2 must fit 2^31 cells");
    if (int rc = bn::open_device(device_id, terrain_fail)) return rc;
    BN_ON_DEVICE(terrain_fail, device_id);
    auto *h = new bn_terrain_t();
    h->device = device_id; h->G = G; h->N = G + 2; h->B = B;
    const int hN = h->N / 2;
    h->nph = (hN + 1) * (hN + 1) + (hN - 1) * (hN - 1);
    if (int rc = terrain_init(h)) {
        bn_terrain_destroy(h);               // leaves the error text as terrain_init set it
        return rc;
    }
    *out = h;
    return BN_OK;
}

void bn_terrain_destroy(bn_terrain_t *h)
{
    if (!h) return;
    bn::DeviceGuard guard(h->device);
    if ((h->generated || h->ev_recorded) && h->ev_done) (void)hipEventSynchronize(h->ev_done);
    for (bn::DeviceBuffers *t : {&h->stage, &h->draw, &h->color, &h->bufs}) t->free_all();
    delete h;
}

/* set_terrain_geometry's parameters: the map resolution, TerrainGeometry's roughness exponent and amplitude gain, is_fractal. */
int bn_terrain_set_geometry(bn_terrain_t *h, double resolution, double roughness_exponent, double amplitude_gain, int32_t is_fractal)
{
    if (!h) return terrain_fail(BN_ERR_INVALID, "null handle");
    if (!(resolution > 0.0) || !std::isfinite(resolution) || !std::isfinite(roughness_exponent) || !std::isfinite(amplitude_gain))
        return terrain_fail(BN_ERR_INVALID, "resolution must be finite and > 0; exponent and gain finite");
    h->resolution = resolution; h->roughness = roughness_exponent; h->gain = amplitude_gain; h->fractal = is_fractal != 0;
    h->have_geometry = true;
    return BN_OK;
}

int bn_terrain_set_draws(bn_terrain_t *h, const float *phases, const int32_t *crater_count, const int32_t *crater_int,
                         const float *crater_val, int32_t max_craters, const float *lin, int64_t lin_len)
{
    if (!h || !phases || !crater_count || !crater_int || !crater_val || !lin) return terrain_fail(BN_ERR_INVALID, "null argument");
    if (max_craters < 1 || lin_len < 1 || lin_len > ((int64_t)1 << 30)) return terrain_fail(BN_ERR_INVALID, "max_craters and lin_len must be >= 1");
    const int N = h->N;
    for (int b = 0; b < h->B; ++b) {
        if (crater_count[b] < 0 || crater_count[b] > max_craters) return terrain_fail(BN_ERR_INVALID, "crater count out of range");
        for (int c = 0; c < crater_count[b]; ++c) {
            const int32_t *ci = crater_int + ((size_t)b * max_craters + c) * 8;
            const int sx = ci[0], sy = ci[1], ex = ci[2], ey = ci[3], psx = ci[4], psy = ci[5], n = ci[6], off = ci[7];
            if (sx < 0 || sy < 0 || ex > N || ey > N || ex < sx || ey < sy || psx < 0 || psy < 0 || n < 1 ||
                psx + (ex - sx) > n || psy + (ey - sy) > n || off < 0 || (int64_t)off + n > lin_len)
                return terrain_fail(BN_ERR_INVALID, "crater " + std::to_string(c) + " of instance " + std::to_string(b) + " is out of range");
        }
    }
    TERRAIN_ON_DEVICE(h);
    int rc = wait_done(h);
    if (rc) return rc;
    if (max_craters != h->maxc && (rc = resize_craters(h, max_craters))) return rc;
    if ((rc = fit_lin(h, lin_len))) return rc;
    TERRAIN_HIP(hipMemcpy(h->phases, phases, (size_t)h->nph * h->B * 4, hipMemcpyHostToDevice));
    TERRAIN_HIP(hipMemcpy(h->cr_count, crater_count, (size_t)h->B * 4, hipMemcpyHostToDevice));
    TERRAIN_HIP(hipMemcpy(h->cr_int, crater_int, (size_t)h->B * max_craters * 32, hipMemcpyHostToDevice));
    TERRAIN_HIP(hipMemcpy(h->cr_val, crater_val, (size_t)h->B * max_craters * 8, hipMemcpyHostToDevice));
    TERRAIN_HIP(hipMemcpy(h->lin, lin, (size_t)lin_len * 4, hipMemcpyHostToDevice));
    h->have_draws = true;
    h->drawn = false;
    return BN_OK;
}

int bn_terrain_set_draw_params(bn_terrain_t *h, int32_t is_crater, int32_t num_craters, double crater_margin, double min_angle,
                               double max_angle, double min_radius, double max_radius, int32_t with_light, double lower_threshold,
                               double upper_threshold)
{
    if (!h) return terrain_fail(BN_ERR_INVALID, "null handle");
    if (!h->have_geometry) return terrain_fail(BN_ERR_STATE, "the geometry (resolution) must be set first");
    if (num_craters < 0 || num_craters > bn::kMaxDrawCraters)
        return terrain_fail(BN_ERR_INVALID, "num_craters must be in [0, " + std::to_string(bn::kMaxDrawCraters) + "], the crater slots of the device draws");
    for (double v : {crater_margin, min_angle, max_angle, min_radius, max_radius, lower_threshold, upper_threshold})
        if (!std::isfinite(v)) return terrain_fail(BN_ERR_INVALID, "the draw parameters must be finite");
    if (!(min_radius > 0.0) || !(max_radius > 0.0)) return terrain_fail(BN_ERR_INVALID, "min_radius and max_radius must be > 0");
    const int slots = std::max(is_crater ? num_craters : 0, 1);
    const double stride = std::ceil(2.0 * std::max(min_radius, max_radius) / h->resolution) + 2.0;
    if (!(stride * slots * h->B <= (double)((int64_t)1 << 30)))
        return terrain_fail(BN_ERR_INVALID, "the crater profiles (B x num_craters x 2 max_radius / resolution) must fit 2^30 values");
    TERRAIN_ON_DEVICE(h);
    h->dr_crater = is_crater != 0; h->dr_num = num_craters; h->dr_light = with_light != 0;
    h->dr_margin = crater_margin; h->dr_amin = min_angle; h->dr_amax = max_angle; h->dr_rmin = min_radius; h->dr_rmax = max_radius;
    h->dr_llo = lower_threshold; h->dr_lhi = upper_threshold;
    h->have_draw_params = true;
    return ensure_draw_buffers(h);
}

int bn_terrain_draw_async(bn_terrain_t *h, const uint64_t *seeds, void *stream)
{
    if (!h || !seeds) return terrain_fail(BN_ERR_INVALID, "null argument");
    if (!h->have_geometry || !h->have_draw_params) return terrain_fail(BN_ERR_STATE, "geometry and draw parameters must be set first");
    if (h->dr_light && !h->light) return terrain_fail(BN_ERR_STATE, "the light source is drawn for the colouring: set it first");
    TERRAIN_ON_DEVICE(h);
    int rc = wait_done(h);                   // the last draws or generation: the staging buffer and the tables are free again
    if (rc || (rc = ensure_draw_buffers(h))) return rc;
    hipStream_t s = (hipStream_t)stream;
    std::memcpy(h->dseeds_pinned, seeds, (size_t)h->B * 8);                  // the caller's seeds are consumed before this returns
    TERRAIN_HIP(hipMemcpyAsync(h->dseeds, h->dseeds_pinned, (size_t)h->B * 8, hipMemcpyHostToDevice, s));
    const double res = h->resolution, x0 = h->G * res / 2 - h->G / 2.0 * res;
    bn::DrawArgs a{};
    a.seeds = h->dseeds; a.phases = h->phases; a.cr_count = h->cr_count; a.cr_int = h->cr_int; a.cr_val = h->cr_val; a.lin = h->lin;
    a.light = h->light; a.rec = h->drec; a.centers = h->dcenters; a.angles = h->dangles; a.light_u = h->dlight_u;
    a.G = h->G; a.N = h->N; a.nph = h->nph; a.maxc = h->maxc; a.stride = (int)draw_stride(h);
    a.want = h->dr_crater ? h->dr_num : 0; a.fractal = h->fractal; a.with_light = h->dr_light;
    a.span = (float)((h->N - 1) * res - x0); a.org = (float)x0; a.res = (float)res;
    a.rspan = (float)(h->dr_rmax - h->dr_rmin); a.rmin = (float)h->dr_rmin; a.margin = (float)h->dr_margin;
    a.lspan = (float)(h->dr_lhi - h->dr_llo); a.llo = (float)h->dr_llo;
    a.aspan = h->dr_amax - h->dr_amin; a.amin = h->dr_amin;
    bn::terrain_draws_kernel<<<h->B, bn::kDrawThreads, 0, s>>>(a);
    TERRAIN_HIP(hipGetLastError());
    TERRAIN_HIP(hipEventRecord(h->ev_done, s));
    h->ev_recorded = true;
    h->have_draws = true;
    h->drawn = true;
    return BN_OK;
}

int bn_terrain_draw_layout(bn_terrain_t *h, int32_t *slots, int32_t *stride)
{
    if (!h || !slots || !stride) return terrain_fail(BN_ERR_INVALID, "null argument");
    if (!h->have_draw_params) return terrain_fail(BN_ERR_STATE, "the draw parameters must be set first");
    *slots = std::max(h->dr_crater ? h->dr_num : 0, 1);
    *stride = (int32_t)draw_stride(h);
    return BN_OK;
}

int bn_terrain_read_draws(bn_terrain_t *h, int32_t *records, float *centers, double *angles, float *light_uniforms, float *light,
                          int32_t *crater_int, float *crater_val, float *lin, float *phases)
{
    if (!h) return terrain_fail(BN_ERR_INVALID, "null handle");
    if (!h->drawn) return terrain_fail(BN_ERR_STATE, "no draws made on the device yet");
    if (h->maxc != h->dr_slots) return terrain_fail(BN_ERR_STATE, "the crater tables were replaced by host draws since the device drew");
    if (light && !h->light) return terrain_fail(BN_ERR_STATE, "colouring has not been set");
    TERRAIN_ON_DEVICE(h);
    int rc = wait_done(h);
    if (rc) return rc;
    const size_t B = (size_t)h->B, slots = (size_t)h->dr_slots;
    if (records) TERRAIN_HIP(hipMemcpy(records, h->drec, B * bn::kDrawRecord * 4, hipMemcpyDeviceToHost));
    if (centers) TERRAIN_HIP(hipMemcpy(centers, h->dcenters, B * slots * 8, hipMemcpyDeviceToHost));
    if (angles) TERRAIN_HIP(hipMemcpy(angles, h->dangles, B * slots * 8, hipMemcpyDeviceToHost));
    if (light_uniforms) TERRAIN_HIP(hipMemcpy(light_uniforms, h->dlight_u, B * 8, hipMemcpyDeviceToHost));
    if (light) TERRAIN_HIP(hipMemcpy(light, h->light, B * 12, hipMemcpyDeviceToHost));
    if (crater_int) TERRAIN_HIP(hipMemcpy(crater_int, h->cr_int, B * slots * 32, hipMemcpyDeviceToHost));
    if (crater_val) TERRAIN_HIP(hipMemcpy(crater_val, h->cr_val, B * slots * 8, hipMemcpyDeviceToHost));
    if (lin) TERRAIN_HIP(hipMemcpy(lin, h->lin, B * slots * (size_t)draw_stride(h) * 4, hipMemcpyDeviceToHost));
    if (phases) TERRAIN_HIP(hipMemcpy(phases, h->phases, B * (size_t)h->nph * 4, hipMemcpyDeviceToHost));
    return BN_OK;
}

int bn_terrain_set_slip(bn_terrain_t *h, const int32_t *t_classes, const float *class_params, int32_t num_classes)
{
    if (!h || (num_classes > 0 && !class_params)) return terrain_fail(BN_ERR_INVALID, "null argument");
    if (num_classes < 0 || num_classes > (1 << 20)) return terrain_fail(BN_ERR_INVALID, "num_classes out of range");
    TERRAIN_ON_DEVICE(h);
    int rc = wait_done(h);
    if (rc) return rc;
    if (num_classes != h->nclass) {
        h->nclass = -1;
        if ((rc = h->bufs.resize(&h->cparams, (size_t)num_classes * bn::kClassParams * 4, terrain_fail))) return rc;
        h->nclass = num_classes;
    }
    if (t_classes) TERRAIN_HIP(hipMemcpy(h->classes, t_classes, (size_t)h->G * h->G * h->B * 4, hipMemcpyHostToDevice));
    if (num_classes > 0)
        TERRAIN_HIP(hipMemcpy(h->cparams, class_params, (size_t)num_classes * bn::kClassParams * 4, hipMemcpyHostToDevice));
    h->have_slip = true;
    return BN_OK;
}

int bn_terrain_generate_async(bn_terrain_t *h, void *stream)
{
    if (!h) return terrain_fail(BN_ERR_INVALID, "null handle");
    if (!h->have_geometry || !h->have_draws || !h->have_slip) return terrain_fail(BN_ERR_STATE, "geometry, draws and slip models must be set first");
    TERRAIN_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    const bn::TerrainArgs a = make_args(h);
    const size_t pc = (size_t)h->N * h->N * h->B, oc = (size_t)h->G * h->G * h->B;
    TERRAIN_HIP(hipMemsetAsync(h->hp, 0, pc * 4, s));
    if (h->coloring) {
        const bn::ColorArgs ca = make_color_args(h);
        if (h->own_noise) {
            bn::terrain_noise_kernel<<<(unsigned)((oc + 255) / 256), 256, 0, s>>>(ca);
            TERRAIN_HIP(hipGetLastError());
        }
        bn::terrain_classes_kernel<<<h->B, bn::kReduceThreads, 0, s>>>(ca);
        TERRAIN_HIP(hipGetLastError());
    }
    bn::terrain_crater_kernel<<<h->B, bn::kReduceThreads, 0, s>>>(a);
    TERRAIN_HIP(hipGetLastError());
    if (h->fractal) {
        bn::terrain_spectrum_kernel<<<(unsigned)((pc + 255) / 256), 256, 0, s>>>(a);
        TERRAIN_HIP(hipGetLastError());
        const dim3 blk(bn::kTile, bn::kTile), grd((h->N + bn::kTile - 1) / bn::kTile, (h->N + bn::kTile - 1) / bn::kTile, h->B);
        bn::terrain_dft_rows_kernel<<<grd, blk, 0, s>>>(a);
        TERRAIN_HIP(hipGetLastError());
        bn::terrain_dft_cols_kernel<<<grd, blk, 0, s>>>(a);
        TERRAIN_HIP(hipGetLastError());
        bn::terrain_minshift_kernel<<<h->B, bn::kReduceThreads, 0, s>>>(a);
        TERRAIN_HIP(hipGetLastError());
    }
    bn::terrain_surface_kernel<<<(unsigned)((oc + 255) / 256), 256, 0, s>>>(a);
    TERRAIN_HIP(hipGetLastError());
    if (h->coloring) {
        bn::terrain_color_kernel<<<(unsigned)((oc + 255) / 256), 256, 0, s>>>(make_color_args(h));
        TERRAIN_HIP(hipGetLastError());
    }
    TERRAIN_HIP(hipEventRecord(h->ev_done, s));
    h->generated = true;
    h->colored = h->coloring;
    return BN_OK;
}

int bn_terrain_sync(bn_terrain_t *h)
{
    if (!h) return terrain_fail(BN_ERR_INVALID, "null handle");
    TERRAIN_ON_DEVICE(h);
    return wait_done(h);
}

int bn_terrain_buffers(bn_terrain_t *h, void **heights, void **slopes, void **mean, void **stddev)
{
    if (!h || !heights || !slopes || !mean || !stddev) return terrain_fail(BN_ERR_INVALID, "null argument");
    *heights = h->heights; *slopes = h->slopes; *mean = h->mean; *stddev = h->stddev;
    return BN_OK;
}

int bn_terrain_copy_out(bn_terrain_t *h, float *heights, float *slopes, float *mean, float *stddev)
{
    if (!h) return terrain_fail(BN_ERR_INVALID, "null handle");
    if (!h->generated) return terrain_fail(BN_ERR_STATE, "nothing generated yet");
    TERRAIN_ON_DEVICE(h);
    int rc = wait_done(h);
    if (rc) return rc;
    const size_t bytes = (size_t)h->G * h->G * h->B * 4;
    if (heights) TERRAIN_HIP(hipMemcpy(heights, h->heights, bytes, hipMemcpyDeviceToHost));
    if (slopes) TERRAIN_HIP(hipMemcpy(slopes, h->slopes, bytes, hipMemcpyDeviceToHost));
    if (mean) TERRAIN_HIP(hipMemcpy(mean, h->mean, bytes, hipMemcpyDeviceToHost));
    if (stddev) TERRAIN_HIP(hipMemcpy(stddev, h->stddev, bytes, hipMemcpyDeviceToHost));
    return BN_OK;
}

int bn_terrain_set_coloring(bn_terrain_t *h, int32_t enable, const float *thresholds, const int32_t *start, int32_t num_classes,
                            const float *color_table, const float *light, float ambient_intensity, float feature_size,
                            const float *noise, const uint64_t *seeds, int32_t num_slip_models)
{
    if (!h) return terrain_fail(BN_ERR_INVALID, "null handle");
    if (!enable) { h->coloring = false; return BN_OK; }
    if (!thresholds || !start || !color_table || !light) return terrain_fail(BN_ERR_INVALID, "null argument");
    if (!noise && !seeds) return terrain_fail(BN_ERR_INVALID, "either a noise field or the seeds of the library's noise are needed");
    if (num_classes < 1 || num_classes > bn::kMaxColorClasses)
        return terrain_fail(BN_ERR_INVALID, "colouring supports 1 to " + std::to_string(bn::kMaxColorClasses) + " terrain classes");
    if (!std::isfinite(ambient_intensity) || !std::isfinite(feature_size) || !(feature_size >= 1e-3f))
        return terrain_fail(BN_ERR_INVALID, "ambient_intensity must be finite and feature_size finite and >= 1e-3");
    for (int b = 0; b < h->B; ++b)
        if (start[b] < 0 || start[b] > num_classes) return terrain_fail(BN_ERR_INVALID, "start class out of range");
    TERRAIN_ON_DEVICE(h);
    int rc = wait_done(h);
    if (rc) return rc;
    if ((rc = ensure_color_buffers(h, num_classes))) return rc;
    const size_t oc = (size_t)h->G * h->G * h->B;
    TERRAIN_HIP(hipMemcpy(h->thr, thresholds, (size_t)h->B * num_classes * 4, hipMemcpyHostToDevice));
    TERRAIN_HIP(hipMemcpy(h->cstart, start, (size_t)h->B * 4, hipMemcpyHostToDevice));
    TERRAIN_HIP(hipMemcpy(h->ctable, color_table, (size_t)num_classes * 12, hipMemcpyHostToDevice));
    TERRAIN_HIP(hipMemcpy(h->light, light, (size_t)h->B * 12, hipMemcpyHostToDevice));
    if (noise) TERRAIN_HIP(hipMemcpy(h->noise, noise, oc * 4, hipMemcpyHostToDevice));
    else TERRAIN_HIP(hipMemcpy(h->cseeds, seeds, (size_t)h->B * 8, hipMemcpyHostToDevice));
    h->own_noise = noise == nullptr;
    h->ambient = ambient_intensity; h->feature = feature_size; h->nmodels = num_slip_models;
    h->coloring = true;
    return BN_OK;
}

int bn_terrain_colorize(bn_terrain_t *h, const float *heights, const int32_t *t_classes, const float *color_table, int32_t num_classes,
                        const float *light, float ambient_intensity, void *stream)
{
    if (!h || !heights || !t_classes || !color_table || !light) return terrain_fail(BN_ERR_INVALID, "null argument");
    if (num_classes < 1 || num_classes > bn::kMaxColorClasses)
        return terrain_fail(BN_ERR_INVALID, "colouring supports 1 to " + std::to_string(bn::kMaxColorClasses) + " terrain classes");
    if (!std::isfinite(ambient_intensity)) return terrain_fail(BN_ERR_INVALID, "ambient_intensity must be finite");
    TERRAIN_ON_DEVICE(h);
    int rc = wait_done(h);
    if (rc) return rc;
    if ((rc = ensure_color_buffers(h, num_classes))) return rc;
    const size_t oc = (size_t)h->G * h->G * h->B;
    if ((rc = h->stage.ensure(terrain_fail))) return rc;
    TERRAIN_HIP(hipMemcpy(h->cz_heights, heights, oc * 4, hipMemcpyHostToDevice));
    TERRAIN_HIP(hipMemcpy(h->cz_classes, t_classes, oc * 4, hipMemcpyHostToDevice));
    TERRAIN_HIP(hipMemcpy(h->ctable, color_table, (size_t)num_classes * 12, hipMemcpyHostToDevice));
    TERRAIN_HIP(hipMemcpy(h->light, light, (size_t)h->B * 12, hipMemcpyHostToDevice));
    bn::ColorArgs a = make_color_args(h);
    a.heights = h->cz_heights; a.classes = h->cz_classes; a.ambient = ambient_intensity;
    hipStream_t s = (hipStream_t)stream;
    bn::terrain_color_kernel<<<(unsigned)((oc + 255) / 256), 256, 0, s>>>(a);
    TERRAIN_HIP(hipGetLastError());
    TERRAIN_HIP(hipEventRecord(h->ev_done, s));
    h->ev_recorded = true;
    return BN_OK;
}

int bn_terrain_color_buffers(bn_terrain_t *h, void **classes, void **colors, void **noise)
{
    if (!h || !classes || !colors || !noise) return terrain_fail(BN_ERR_INVALID, "null argument");
    if (!h->colors) return terrain_fail(BN_ERR_STATE, "colouring has not been set");
    *classes = h->classes; *colors = h->colors; *noise = h->noise;
    return BN_OK;
}

int bn_terrain_class_counts(bn_terrain_t *h, int32_t *unassigned, int32_t *beyond)
{
    if (!h || !unassigned || !beyond) return terrain_fail(BN_ERR_INVALID, "null argument");
    if (!h->generated || !h->colored || !h->counts) return terrain_fail(BN_ERR_STATE, "no coloured generation yet");
    TERRAIN_ON_DEVICE(h);
    int rc = wait_done(h);
    if (rc) return rc;
    std::vector<int32_t> c((size_t)h->B * 2);
    TERRAIN_HIP(hipMemcpy(c.data(), h->counts, c.size() * 4, hipMemcpyDeviceToHost));
    for (int b = 0; b < h->B; ++b) { unassigned[b] = c[2 * b]; beyond[b] = c[2 * b + 1]; }
    return BN_OK;
}

int bn_terrain_spectrum(bn_terrain_t *h, int32_t inst, float *out)
{
    if (!h || !out) return terrain_fail(BN_ERR_INVALID, "null argument");
    if (inst < 0 || inst >= h->B) return terrain_fail(BN_ERR_INVALID, "instance out of range");
    if (!h->have_geometry || !h->have_draws) return terrain_fail(BN_ERR_STATE, "geometry and draws must be set first");
    TERRAIN_ON_DEVICE(h);
    int rc = wait_done(h);
    if (rc) return rc;
    const int cells = h->N * h->N;
    float2 *d = nullptr;
    TERRAIN_HIP(hipMalloc((void **)&d, (size_t)cells * 8));
    bn::terrain_spectrum_one_kernel<<<(cells + 255) / 256, 256>>>(make_args(h), inst, d);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(out, d, (size_t)cells * 8, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return terrain_fail(BN_ERR_HIP, std::string("spectrum hook: ") + hipGetErrorString(e));
    return BN_OK;
}

}  // extern "C"
