// mppi_geometry.h -- the cell index of a position, the reachable window of the map in LDS, and the traversability lookups.
#pragma once
#include "mppi_kernels.h"
#include "bn_device_math.h"
#include <math.h>

namespace bn {

namespace {

// Geometry specialisations of the cell index ((p - origin) / res).floor().int()  (grid_map.py:195-209):
//   kGeoGeneral  true division            kGeoPow2  res is a power of two: * (1/res) is bit-identical
//   kGeoPow2Origin0  additionally origin == 0, so the subtraction is the identity
enum Geo : int { kGeoGeneral = 0, kGeoPow2 = 1, kGeoPow2Origin0 = 2 };

struct Win { int wx0, wy0; float fx0, fy0, fwn, fwm1; int wn;
             // the latency kernel's chain wave: constants it keeps in vector registers of its own -- left to the compiler
             // they are re-materialised from scalar registers in every chunk
             float xhi_v, yhi_v; v2f c0_v; };   // window origin (cells), as floats, edge, edge-1, edge

template <int GEO>
__device__ __forceinline__ int raw_cell(float v, float origin, float res, float inv_res)
{
    const float q = (GEO == kGeoPow2Origin0) ? v * inv_res : (GEO == kGeoPow2) ? (v - origin) * inv_res : (v - origin) / res;
    return (int)floorf(q);                    // v_cvt_i32_f32 saturates
}

// (p - origin) / res for a resolution that is not a power of two, as the reference rounds it (a true division, grid_map.py:203), for
// the in-loop lookups: d >= 0 is a clamped position minus the lower limit.  With r = RN(1 / res) (the host's correctly rounded
// reciprocal) q0 = d r, e = fma(-q0, res, d) (the exact residual), q = fma(e, r, q0) is the correctly rounded quotient (Markstein's
// correction step): three packed instructions where the IEEE expansion of two divisions is twenty-two.  No branch back to the
// division here (it cost the chain 1.4 us per solve, tools/res_rate.py): bn_mppi_create checks the form EXHAUSTIVELY on the device
// -- every float d in [0, upper limit - lower limit]: same floor as d / res, same bits above the denormal range -- and refuses a
// resolution that fails (none known: a host sweep over resolutions incl. all-ones significands, the theorem's exception, found no
// mismatch above 1e-30).  K=1024, T=50 at res 0.3: 13.1 (division) -> 10.0 us per solve; res 0.5 (exact multiply): 8.7.
__device__ __forceinline__ v2f quotient_general(const SolveParams &p, v2f d)
{
    const v2f r = {p.inv_res, p.inv_res}, b = {p.res, p.res};
    const v2f q0 = d * r;
    const v2f e = __builtin_elementwise_fma(-q0, b, d);
    return __builtin_elementwise_fma(e, r, q0);
}

// Window of edge wn covering `reach` cells either side of the cell of (sx, sy) and one more above, shifted into the map PLUS ONE
// GUARD ROW / COLUMN at index G (staged as a copy of row / column G-1): a position on the upper map limit has the raw cell G, and
// the reference's index clamp (grid_map.py:209) is then built into the window instead of costing the chain two clamps a step.
template <int GEO>
__device__ __forceinline__ Win window_origin_wide(const SolveParams &p, float sx, float sy, int reach, int wn)
{
    const int cx = clampi(raw_cell<GEO>(sx, p.x0, p.res, p.inv_res), 0, p.G - 1);
    const int cy = clampi(raw_cell<GEO>(sy, p.y0, p.res, p.inv_res), 0, p.G - 1);
    Win w;
    w.wx0 = min(max(cx - reach, 0), p.G + 1 - wn);
    w.wy0 = min(max(cy - reach, 0), p.G + 1 - wn);
    w.fx0 = (float)w.wx0; w.fy0 = (float)w.wy0; w.fwn = (float)wn; w.fwm1 = (float)(wn - 1); w.wn = wn;
    return w;
}

template <int GEO>
__device__ __forceinline__ Win window_origin(const SolveParams &p, float sx, float sy)
{
    return window_origin_wide<GEO>(p, sx, sy, p.reach, p.WN);
}

// Stage the reachable window as traversability: trav = 1 - clamp(risk, 0, 1)
// (reference traversability_model.py:72).  Rows of the window are contiguous
// runs of the map rows, so the loads coalesce per row.
__device__ __forceinline__ void stage_window(float *win, const float *__restrict__ map, const Win w,
                                             int WN, int G, int tid, int nthreads)
{
    // Four cells per thread and round trip: written as one cell per iteration the loop is load - wait - store, a full memory round trip
    // per 320 cells, in the prologue of every launch and of every tail (round 5: the headline's 24 x 24 window took two).
    const int n = WN * WN;
    for (int e0 = tid; e0 < n; e0 += 4 * nthreads) {
        float risk[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = min(e0 + i * nthreads, n - 1);       // (behind the window: the last cell again, not stored)
            const int r = e / WN;
            const int c = e - r * WN;
            risk[i] = map[(size_t)min(w.wy0 + r, G - 1) * G + min(w.wx0 + c, G - 1)];      // (the guard row / column: index G -> G-1)
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = e0 + i * nthreads;
            if (e < n) win[e] = 1.0f - clampf(risk[i], 0.0f, 1.0f);
        }
    }
}

// Traversability at (x, y): index clamp (grid_map.py:209) then the gather.  With the LDS window the
// two clamps (map, then window) collapse into one: the window lies inside the map, so clamping
// i - wx0 to [0, WN-1] gives the same cell for every i (in, left of, or right of the map).
// SAFE additionally bounds the raw index first, for a caller-supplied start state of any magnitude.
template <int GEO, bool LDSWIN, bool SAFE>
__device__ __forceinline__ float trav_lookup(const SolveParams &p, const float *win,
                                             const float *__restrict__ map, const Win w, float x, float y)
{
    int ix, iy;
    if (GEO == kGeoGeneral && !SAFE) {                 // in-loop lookup of a clamped position: the validated three-instruction quotient
        const v2f q = quotient_general(p, v2f{x, y} - v2f{p.x0, p.y0});
        ix = (int)floorf(q.x); iy = (int)floorf(q.y);
    } else {
        ix = raw_cell<GEO>(x, p.x0, p.res, p.inv_res);
        iy = raw_cell<GEO>(y, p.y0, p.res, p.inv_res);
    }
    if (LDSWIN) {
        if (SAFE) { ix = clampi(ix, 0, p.G - 1); iy = clampi(iy, 0, p.G - 1); }
        const int li = clampi(ix - w.wx0, 0, p.WN - 1);
        const int lj = clampi(iy - w.wy0, 0, p.WN - 1);
        return win[(int)__umul24((unsigned)lj, (unsigned)p.WN) + li];
    }
    ix = clampi(ix, 0, p.G - 1);
    iy = clampi(iy, 0, p.G - 1);
    return 1.0f - clampf(map[(size_t)iy * p.G + ix], 0.0f, 1.0f);
}

// In-loop gather: (x, y) already lies inside the map limits and within `reach` cells of the start, so its raw cell lies inside
// the window (guard row / column included: window_origin_wide) and nothing has to be clamped.  q = (x - origin)/res as the
// reference rounds it, then q - wx0 (exact: an integer no larger than q is subtracted), floor, row * WN + col in the float domain
// (exact small integers), one conversion.  Same cell as trav_lookup<..., false> for every such position; six instructions before
// the ds_read where floor, clamp, floor, clamp, fma, convert, shift-add were eight -- on the chain wave they sit on the solve's
// critical path T times.
template <int GEO, int ASMIDX = 0>
__device__ __forceinline__ float trav_window(const SolveParams &p, const float *win, const Win w, float x, float y)
{
    v2f q;
    const v2f xy = {x, y}, ir = {p.inv_res, p.inv_res}, nw = {-w.fx0, -w.fy0};
    if (GEO == kGeoPow2Origin0) {
        q = __builtin_elementwise_fma(xy, ir, nw);                      // one v_pk_fma_f32
    } else if (GEO == kGeoPow2) {
        q = __builtin_elementwise_fma(xy - v2f{p.x0, p.y0}, ir, nw);
    } else {
        q = quotient_general(p, xy - v2f{p.x0, p.y0}) + nw;
    }
    if (ASMIDX == 2 && GEO != kGeoGeneral) {
        // The latency kernel's chain wave (ASMIDX = 2; the tail's X* rollout keeps ASMIDX = 1 below: fixed registers at the top of
        // a 128-register budget would cost the role kernel, whose aux workgroup runs that tail, its occupancy).  The same five instructions -- quotient (packed FMA), floor-and-convert x 2, row * WN + col, byte address -- as ONE asm
        // block whose only result is consumed by the LDS read.  Why: LLVM's hazard recogniser (gfx940+ "dst_sel forwarding") puts
        // an s_nop between (a) any VALU consumer and an inline asm that defines its operand and (b) an inline asm and a packed
        // instruction with op_sel_hi[0] = 1 that defines one of its operands (the bit shares its position with VOP3's dst op_sel:
        // a false positive for VOP3P).  The old cut -- packed FMA | asm(cvt, cvt, mad) | shift-add -- paid both, two issue slots
        // of the chain wave per step.  Inside one block there is no hazard to assume, and a DS consumer is not a VALU consumer.
        // v126 / v127: scratch (the halves of a 64-bit asm operand cannot be named, so the quotient lives in fixed registers).
        typedef __attribute__((address_space(3))) const float lds_cf;
        const unsigned base = (unsigned)(uintptr_t)(lds_cf *)win;
        const v2f xyo = GEO == kGeoPow2Origin0 ? xy : xy - v2f{p.x0, p.y0};
        unsigned addr;
        asm("v_pk_fma_f32 v[126:127], %1, %2, %3\n\t"
            "v_cvt_flr_i32_f32 v126, v126\n\t"
            "v_cvt_flr_i32_f32 v127, v127\n\t"
            "v_mad_u32_u24 v126, v127, %4, v126\n\t"
            "v_lshl_add_u32 %0, v126, 2, %5"
            : "=v"(addr) : "v"(xyo), "s"(ir), "v"(nw), "s"(w.wn), "s"(base) : "v126", "v127");
        return *(lds_cf *)(uintptr_t)addr;
    }
    if (ASMIDX == 1 || ASMIDX == 3) {
        // The latency kernel's chain wave: floor-and-convert in one instruction, row * WN + col as one v_mad_u32_u24 (left to itself
        // the compiler spreads the *4 of the byte address over both terms).  Same integers.  8.65 -> 8.57 us per dependent solve;
        // NOT for the role kernel (64 instances: +3 %): the compiler pads both ends of an asm block with a wait state and cannot
        // schedule across it.
        int cell, lj;
        asm("v_cvt_flr_i32_f32 %0, %2\n\tv_cvt_flr_i32_f32 %1, %3\n\tv_mad_u32_u24 %0, %1, %4, %0"
            : "=&v"(cell), "=&v"(lj) : "v"(q.x), "v"(q.y), "s"(w.wn));
        return win[cell];
    }
    return win[(int)__builtin_fmaf(floorf(q.y), w.fwn, floorf(q.x))];
}

}  // namespace

}  // namespace bn
