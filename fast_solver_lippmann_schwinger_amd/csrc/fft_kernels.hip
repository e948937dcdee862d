// Pruned, fused axis passes of the padded-grid convolution (gfx950).
//
//   y = alpha*x + beta * crop( IFFT( sym .* FFT( pad( nu .* x ) ) ) )
//
// on the reduced grid Lx x Ly x Lz = 2n x 2m x 2l, never touching the zero 7/8 of
// the padded cube (35 complex + 1 real of HBM traffic per point):
//
//   xfwd   x[n][m][l] (*nu)            -> A1[Lx][m][l]            lines contiguous
//   yfwd   A1                          -> A2[8][l][Ly][Lx/8]      128-B chunks in, 128-B chunks out
//   zfused A2 (in place) .* sym        -> A2                      fully contiguous 8-line tiles
//   yinv   A2                          -> A1[Lx][m][l]
//   xinv   A1, x                       -> y[n][m][l]
//
// (2D: xfwd -> zfused along y on the natural A1[Lx][m] -> xinv.)
// The grid sizes n, m, l need not be powers of two: every pass reads only the first n (m, l) entries of a line
// and zero-fills up to L/2, writes only the first n (m, l) on the way back; L = pruned_best_length(n) per axis.
// Frequency-side indices are "storage" indices (fft_core.hpp); A2 is tiled so that
// the eight x'-neighbours of a z-line are interleaved (xi fastest), which makes
// the largest pass (z: 16 of the 35 complex per point) a pure stream.
#include "common.hpp"
#include "fft_configs.hpp"
#include "pruned.hpp"
#include <cstdlib>
#include <mutex>
#include <set>
#include <map>
#include <utility>
#include <cstring>

// This file is compiled once per family of line lengths (Makefile: -DLSFC_FAMILY=2 | 3 | 5): the power-of-two lines,
// the lines with one factor 3 and the lines with one factor 5.  pruned.hip routes each call to the family of its L.
#ifndef LSFC_FAMILY
#error "compile with -DLSFC_FAMILY=2, 3 or 5"
#endif
#define LSFC_CAT2(a, b) a##b
#define LSFC_CAT(a, b) LSFC_CAT2(a, b)
#define FAM(name) LSFC_CAT(LSFC_CAT(name, _f), LSFC_FAMILY)

namespace lsfc {
using namespace fft;

static constexpr int XB = 8;           // x' lines per strided workgroup: 8 * 16 B = one 128-B line

// EXACT: n == L/2 (the grid fills the line): the end-of-line predicates compile away
template <class C, int LPW, bool SPLIT, bool EXACT>
__global__ __launch_bounds__(C::T * LPW)
void k_xfwd(const VecBatch vb, int64_t obatch, const double* __restrict__ nu, cplx* __restrict__ out,
            const cplx* __restrict__ tw, int64_t nlines, int wmagic, int W, int Wp, int n, int64_t bstride, int cj) {
    // blockIdx.y = right-hand side of the batch
    const cplx* __restrict__ x = vb.x[blockIdx.y];
    out += (int64_t)blockIdx.y * obatch;
    using LL = LdsLayout<1, 3, SPLIT>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int T = C::T, E = C::E;
    const int t = threadIdx.x % T, ll = threadIdx.x / T;
    const int64_t line = (int64_t)blockIdx.x * LPW + ll;
    const bool valid = line < nlines;
    const int64_t lc = valid ? line : nlines - 1;
    const cplx* xin = x + lc * n;
    cplx v[E];
#pragma unroll
    for (int e = 0; e < E / 2; ++e) v[e] = (EXACT || t + T * e < n) ? xin[t + T * e] : make_double2(0.0, 0.0);
    if (nu) {
        const double* nin = nu + lc * n;
#pragma unroll
        for (int e = 0; e < E / 2; ++e) { const double s = (EXACT || t + T * e < n) ? nin[t + T * e] : 0.0; v[e].x *= s; v[e].y *= s; }
    }
    // cj (a kernel argument, like nu: one scalar branch per wave): the transform of conj(x), for the adjoint operator
    if (cj) {
#pragma unroll
        for (int e = 0; e < E / 2; ++e) v[e].y = -v[e].y;
    }
#pragma unroll
    for (int e = E / 2; e < E; ++e) v[e] = make_double2(0.0, 0.0);
    fft_forward<C, LL, true>(v, t, tw, smem, ll * LL::line_elems(C::L), 0);
    if (valid) {
        // storage index s of this line goes to chunk s / W (one chunk per destination rank and pipeline stage of the
        // slab transpose; a single chunk of width L on one GPU): out[chunk][line][s % W], row pitch Wp >= W.  The
        // division is exact by multiplication: wmagic = floor(2^22 / W) + 1, valid for s < 2048.
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int s = t + T * e;
            const int c = (int)(((unsigned)s * (unsigned)wmagic) >> 22);
            out[(int64_t)c * bstride + line * Wp + (s - c * W)] = v[e];
        }
    }
}

template <class C, int LPW, bool SPLIT, bool EXACT>
__global__ __launch_bounds__(C::T * LPW)
void k_xinv(const cplx* __restrict__ in, const VecBatch vb, int64_t ibatch, double alpha, double beta,
            const cplx* __restrict__ tw, int64_t nlines, int wmagic, int W, int Wp, int n, int64_t bstride,
            const double* nu, int cj) {
    const cplx* xorig = vb.x[blockIdx.y];
    cplx* y = vb.y[blockIdx.y];
    in += (int64_t)blockIdx.y * ibatch;
    using LL = LdsLayout<1, 3, SPLIT>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int T = C::T, E = C::E;
    const int t = threadIdx.x % T, ll = threadIdx.x / T;
    const int64_t line = (int64_t)blockIdx.x * LPW + ll;
    const bool valid = line < nlines;
    const int64_t lc = valid ? line : nlines - 1;
    cplx v[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int s = t + T * e;
        const int c = (int)(((unsigned)s * (unsigned)wmagic) >> 22);
        v[e] = in[(int64_t)c * bstride + lc * Wp + (s - c * W)];
    }
    fft_inverse<C, LL, true>(v, t, tw, smem, ll * LL::line_elems(C::L), 0);
    // y = alpha*x + beta * nu .* (conj) v: nu (the transposed operator; NOT __restrict__, like x it is read at the very index this
    // thread then stores to) and cj are kernel arguments, as alpha is -- scalar branches, and with neither the arithmetic below
    // is what it was (beta * v)
    if (cj) {
#pragma unroll
        for (int e = 0; e < E / 2; ++e) v[e].y = -v[e].y;
    }
    if (valid) {
#pragma unroll
        for (int e = 0; e < E / 2; ++e) {
            if (EXACT || t + T * e < n) {
                const int64_t idx = line * n + t + T * e;
                const double bs = nu ? beta * nu[idx] : beta;
                cplx r = make_double2(bs * v[e].x, bs * v[e].y);
                if (alpha != 0.0) { const cplx xo = xorig[idx]; r.x = fma(alpha, xo.x, r.x); r.y = fma(alpha, xo.y, r.y); }
                y[idx] = r;
            }
        }
    }
}

// The x passes of a plan whose nu is complex (lsfc_plan_set_nu_complex): kernels of their own, so that k_xfwd and k_xinv above are,
// instruction for instruction, what they were before there was a complex nu.  Same template arguments, same forms, same launch
// geometry and LDS; nu (the real plane) and nu_im (the imaginary one) are both non-null here.  The conjugation is outermost
// (plan.hpp, ConvOp): with cj the input pass hands G the vector nu .* conj(x) = conj(conj(nu) .* x), the output pass stores
// conj(nu) .* conj(v).  The imaginary loads use the end-of-line predicate and the clamped line index of the real ones.
template <class C, int LPW, bool SPLIT, bool EXACT>
__global__ __launch_bounds__(C::T * LPW)
void k_xfwd_c(const VecBatch vb, int64_t obatch, const double* __restrict__ nu, const double* __restrict__ nu_im, cplx* __restrict__ out,
              const cplx* __restrict__ tw, int64_t nlines, int wmagic, int W, int Wp, int n, int64_t bstride, int cj) {
    const cplx* __restrict__ x = vb.x[blockIdx.y];
    out += (int64_t)blockIdx.y * obatch;
    using LL = LdsLayout<1, 3, SPLIT>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int T = C::T, E = C::E;
    const int t = threadIdx.x % T, ll = threadIdx.x / T;
    const int64_t line = (int64_t)blockIdx.x * LPW + ll;
    const bool valid = line < nlines;
    const int64_t lc = valid ? line : nlines - 1;
    const cplx* xin = x + lc * n;
    const double* nin = nu + lc * n;
    const double* iin = nu_im + lc * n;
    cplx v[E];
#pragma unroll
    for (int e = 0; e < E / 2; ++e) {
        const bool in = EXACT || t + T * e < n;
        const cplx xv = in ? xin[t + T * e] : make_double2(0.0, 0.0);
        const double a = in ? nin[t + T * e] : 0.0, b = in ? iin[t + T * e] : 0.0;
        const double xr = xv.x, xi = cj ? -xv.y : xv.y;
        v[e] = make_double2(fma(-b, xi, a * xr), fma(b, xr, a * xi));
    }
#pragma unroll
    for (int e = E / 2; e < E; ++e) v[e] = make_double2(0.0, 0.0);
    fft_forward<C, LL, true>(v, t, tw, smem, ll * LL::line_elems(C::L), 0);
    if (valid) {
        // (the chunked store of k_xfwd)
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int s = t + T * e;
            const int c = (int)(((unsigned)s * (unsigned)wmagic) >> 22);
            out[(int64_t)c * bstride + line * Wp + (s - c * W)] = v[e];
        }
    }
}

template <class C, int LPW, bool SPLIT, bool EXACT>
__global__ __launch_bounds__(C::T * LPW)
void k_xinv_c(const cplx* __restrict__ in, const VecBatch vb, int64_t ibatch, double alpha, double beta,
              const cplx* __restrict__ tw, int64_t nlines, int wmagic, int W, int Wp, int n, int64_t bstride,
              const double* nu, const double* nu_im, int cj) {
    const cplx* xorig = vb.x[blockIdx.y];
    cplx* y = vb.y[blockIdx.y];
    in += (int64_t)blockIdx.y * ibatch;
    using LL = LdsLayout<1, 3, SPLIT>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int T = C::T, E = C::E;
    const int t = threadIdx.x % T, ll = threadIdx.x / T;
    const int64_t line = (int64_t)blockIdx.x * LPW + ll;
    const bool valid = line < nlines;
    const int64_t lc = valid ? line : nlines - 1;
    cplx v[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int s = t + T * e;
        const int c = (int)(((unsigned)s * (unsigned)wmagic) >> 22);
        v[e] = in[(int64_t)c * bstride + lc * Wp + (s - c * W)];
    }
    fft_inverse<C, LL, true>(v, t, tw, smem, ll * LL::line_elems(C::L), 0);
    // y = alpha*x + beta * nu .* v, with cj beta * conj(nu) .* conj(v); nu and nu_im, like x, are read at the very index this thread
    // then stores to (not __restrict__)
    if (valid) {
#pragma unroll
        for (int e = 0; e < E / 2; ++e) {
            if (EXACT || t + T * e < n) {
                const int64_t idx = line * n + t + T * e;
                const double vr = v[e].x, vi = cj ? -v[e].y : v[e].y;
                const double br = beta * nu[idx], bi = cj ? -(beta * nu_im[idx]) : beta * nu_im[idx];
                cplx r = make_double2(fma(-bi, vi, br * vr), fma(bi, vr, br * vi));
                if (alpha != 0.0) { const cplx xo = xorig[idx]; r.x = fma(alpha, xo.x, r.x); r.y = fma(alpha, xo.y, r.y); }
                y[idx] = r;
            }
        }
    }
}

// (two 512-thread workgroups of the y passes per CU -- 128 registers, split exchanges, chained twiddle powers, no spills -- change
// nothing at 512^3: yfwd 2.53 -> 2.51 ms, profiles/r02_experiment_ticketed_half_tiles.log; the passes are bound by their access pattern)
// A1[Lx][m][l] (natural) -> A2[XB][l][Ly][Lx/XB]
template <class C, int LINES, bool SPLIT, int WPE, bool EXACT>
__global__ __launch_bounds__(C::T * LINES, WPE)
void k_yfwd(const cplx* __restrict__ a1, cplx* __restrict__ a2, const cplx* __restrict__ tw, int Lx, int m, int l, int TG, int TZ, int p1, int p2,
            int64_t batch1, int64_t batch2) {
    using LL = LdsLayout<LINES, 3, SPLIT>;
    a1 += (int64_t)blockIdx.y * batch1; a2 += (int64_t)blockIdx.y * batch2;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int T = C::T, E = C::E, Ly = C::L;
    const int xi = threadIdx.x % LINES, t = threadIdx.x / LINES;
    const int ngrp = Lx / LINES;
    // block order: (TG x TZ) tiles of (x'-group, z), groups fastest inside a tile and across tiles, so that the
    // workgroups in flight together touch short contiguous runs in BOTH the natural and the tiled array
    const int within = blockIdx.x % (TG * TZ), tile = blockIdx.x / (TG * TZ);
    const int ntg = ngrp / TG;
    const int g = (tile % ntg) * TG + within % TG, z = (tile / ntg) * TZ + within / TG;
    const int xp = g * LINES + xi;                       // x' storage index
    const cplx* src = a1 + xp + (int64_t)p1 * m * z;
    cplx v[E];
#pragma unroll
    for (int e = 0; e < E / 2; ++e) v[e] = (EXACT || t + T * e < m) ? src[(int64_t)p1 * (t + T * e)] : make_double2(0.0, 0.0);
#pragma unroll
    for (int e = E / 2; e < E; ++e) v[e] = make_double2(0.0, 0.0);
    fft_forward<C, LL, true, false, (C::T * LINES > 512)>(v, t, tw, smem, 0, xi);     // (1024-thread workgroups, 128 registers: chained twiddle powers, no spills)
    const int xb = xp / XB, xq = xp % XB;
    cplx* dst = a2 + xq + (int64_t)XB * z + (int64_t)p2 * ((int64_t)Ly * xb);
#pragma unroll
    for (int e = 0; e < E; ++e) dst[(int64_t)p2 * (t + T * e)] = v[e];
}

template <class C, int LINES, bool SPLIT, int WPE, bool EXACT>
__global__ __launch_bounds__(C::T * LINES, WPE)
void k_yinv(const cplx* __restrict__ a2, cplx* __restrict__ a1, const cplx* __restrict__ tw, int Lx, int m, int l, int TG, int TZ, int p1, int p2,
            int64_t batch1, int64_t batch2) {
    using LL = LdsLayout<LINES, 3, SPLIT>;
    a1 += (int64_t)blockIdx.y * batch1; a2 += (int64_t)blockIdx.y * batch2;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int T = C::T, E = C::E, Ly = C::L;
    const int xi = threadIdx.x % LINES, t = threadIdx.x / LINES;
    const int ngrp = Lx / LINES;
    // block order: (TG x TZ) tiles of (x'-group, z), groups fastest inside a tile and across tiles, so that the
    // workgroups in flight together touch short contiguous runs in BOTH the natural and the tiled array
    const int within = blockIdx.x % (TG * TZ), tile = blockIdx.x / (TG * TZ);
    const int ntg = ngrp / TG;
    const int g = (tile % ntg) * TG + within % TG, z = (tile / ntg) * TZ + within / TG;
    const int xp = g * LINES + xi;
    const int xb = xp / XB, xq = xp % XB;
    const cplx* src = a2 + xq + (int64_t)XB * z + (int64_t)p2 * ((int64_t)Ly * xb);
    cplx v[E];
#pragma unroll
    for (int e = 0; e < E; ++e) v[e] = src[(int64_t)p2 * (t + T * e)];
    fft_inverse<C, LL, true, false, (C::T * LINES > 512)>(v, t, tw, smem, 0, xi);
    cplx* dst = a1 + xp + (int64_t)p1 * m * z;
#pragma unroll
    for (int e = 0; e < E / 2; ++e) if (EXACT || t + T * e < m) dst[(int64_t)p1 * (t + T * e)] = v[e];
}

// In-place forward -> .* sym -> inverse along one strided axis.
// Line (g, outer, xi): element j at data[g*dGrp + outer*dOuter + xi + dLine*j],
// symbol entry for storage index s at sym[g*sGrp + outer*sOuter + xi + sLine*s].
// PREFETCH: the symbol loads are issued before the forward transform, so their HBM latency hides behind its
// butterflies (+E complex registers; pays at E = 16 where the kernel runs at 2 waves/SIMD either way).
// Tried and dropped (profiles/r01_experiment_*.log): LDS-only exchange barriers, non-temporal accesses, a persistent
// software-pipelined form of all five kernels, 128-register builds (two 512-thread workgroups per CU), an
// 8-elements-per-thread four-stage factorisation of the 1024-point line, and Infinity-Cache slab blocking of the
// y/z/y passes -- each measured slower or neutral on MI355X.
// HALF: the workgroup transforms only 4 of the 8 interleaved lines of a tile (64 B of every 128-B line); the two
// halves of a tile are blocks b and b+8 of a group of 16, i.e. (by the observed round-robin placement) on the SAME
// XCD, whose L2 merges their reads and writes of the shared lines.  Halving the workgroup to 4 waves lets two (or
// three) independent workgroups share a CU at the same register budget, so one computes while the other waits on HBM.
// ZE (z-even symbol): a symbol line stores only the entries with frequency kz <= L/2 -- L/2 of them in storage order
// (exactly the slots e < E/2 of every thread) plus the kz = L/2 entry at index L/2.  Each thread loads its E/2
// values; the mirror values (kz -> L - kz) of its slots e >= E/2 are held by other threads of the same line and are
// fetched through LDS (zm[s - L/2] = storage index of the partner).  Halves the symbol bytes of the pass again.
// TWL: the full stage-twiddle table (tw points to it) is staged in LDS behind the exchange buffer and read instead of
// computing the power trees (-18 % fp64 instructions, +40 % LDS reads).
// Whether the one-tile kernel of LINES lines exchanges between stages of equal radix through the lanes of the wavefront (whole-complex
// exchanges, whole wavefronts only).  One definition for the kernel (XL1) and for the description of the pass (PassForm::xl).
template <class C, int LINES, bool SPLIT> constexpr bool xl_one_tile() {
#ifdef LSFC_NO_XLANE_ONE_TILE
    return false;
#else
    return !SPLIT && xlane_ok<C, LdsLayout<LINES, 3, SPLIT>>() && (C::T * LINES) % 64 == 0;
#endif
}
// MULTI (several right-hand sides, lsfc_apply_batch): the workgroup runs the tile of every batch member in turn with
// ONE load of its symbol tile -- the symbol's share of the pass (8 of 16 complex per point in the byte model, 4 with
// the half symbol) is paid once per batch instead of once per right-hand side.
template <class C, int LINES, bool SPLIT, bool PREFETCH, int WPE, bool HALF, bool ZE, bool EXACT, bool TWL, bool MULTI = false>
__global__ __launch_bounds__(C::T * LINES, WPE)
void k_zfused(cplx* __restrict__ data, const cplx* __restrict__ sym, const cplx* __restrict__ tw,
              int nouter, int64_t dGrp, int64_t dOuter, int64_t dLine, int64_t sGrp, int64_t sOuter, int64_t sLine,
              const int2* __restrict__ ytab, const int* __restrict__ zm, int nin, int nrhs, int64_t dBatch, int sibling_pairs) {
    using LL = LdsLayout<LINES, 3, SPLIT>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int T = C::T, E = C::E;
    int xi = threadIdx.x % LINES; const int t = threadIdx.x / LINES;
    unsigned tile = blockIdx.x;
    if constexpr (HALF) {
        // groups of 8 tiles x (XB / LINES) parts: the parts of a tile are 8 blocks apart, i.e. on one XCD
        constexpr int PARTS = XB / LINES, SH = PARTS == 4 ? 5 : 4;
        const unsigned b = blockIdx.x;
        tile = (b >> SH) * 8 + (b & 7);
        xi += (int)((b >> 3) & (PARTS - 1)) * LINES;
    } else if (sibling_pairs) {
        // 2D layout, 4-line sub-groups: groups 2p and 2p + 1 are the two halves of the same 128-B lines.  Blocks b and b + 8
        // (same XCD under round-robin placement) take them, so one L2 fetches each line once instead of two L2s once each.
        const unsigned b = blockIdx.x;
        tile = (((b >> 4) * 8 + (b & 7)) << 1) | ((b >> 3) & 1);
    }
    // block order -> (data row, symbol row): with a y-even symbol a row and its mirror share one symbol row and sit
    // next to each other in block order, so the second read of that row is served by the Infinity Cache, not HBM
    const int o = tile % nouter, g = tile / nouter;
    int outer = o, srow = o;
    if (ytab) { const int2 e = ytab[o]; outer = e.x; srow = e.y; }
    cplx* d = data + g * dGrp + outer * dOuter + xi;
    const cplx* s = sym + g * sGrp + srow * sOuter + xi;
    const int li = threadIdx.x % LINES;                 // line slot inside this workgroup's LDS
    if constexpr (TWL) {
        cplx* tl = reinterpret_cast<cplx*>(smem + (size_t)LL::line_elems(C::L) * LINES * LL::elem_bytes());
        for (int i = threadIdx.x; i < C::TWLEN; i += C::T * LINES) tl[i] = tw[i];
        __syncthreads();
        tw = tl;
    }
    // (whole-complex layouts: exchange stores issued from inside the stages, fft_core.hpp)
    // ... and the exchanges between stages of equal radix through the lanes of the wavefront where the line and the layout allow it
    // (fft_core.hpp xlane_stage_ok; whole wavefronts only): one LDS round trip and two workgroup barriers less per direction in a
    // kernel that is a chain of latencies on the small grids and in 2D
    constexpr bool XL1 = xl_one_tile<C, LINES, SPLIT>();
    auto fwd = [&](cplx (&w)[E]) {
        if constexpr (!SPLIT) fft_forward_ws<C, LL, true, TWL, false, XL1>(w, t, tw, smem, 0, li, [] {});
        else fft_forward<C, LL, true, TWL>(w, t, tw, smem, 0, li);
    };
    auto inv = [&](cplx (&w)[E]) {
        if constexpr (!SPLIT) fft_inverse_ws<C, LL, true, TWL, false, XL1>(w, t, tw, smem, 0, li);
        else fft_inverse<C, LL, true, TWL>(w, t, tw, smem, 0, li);
    };
    cplx v[E];
    if constexpr (MULTI) {
        // symbol tile once, then every right-hand side of the batch
        constexpr int H = ZE ? E / 2 : E;
        cplx sv[H];
#pragma unroll
        for (int e = 0; e < H; ++e) sv[e] = s[sLine * (t + T * e)];
        int part[ZE ? H : 1];
        cplx smid = make_double2(0.0, 0.0);
        if constexpr (ZE) {
#pragma unroll
            for (int e = 0; e < H; ++e) part[e] = zm[t + T * e];
            if (t == 0) smid = s[sLine * (C::L / 2)];
        }
        for (int r = 0; r < nrhs; ++r) {
            cplx* dr = d + (int64_t)r * dBatch;
#pragma unroll
            for (int e = 0; e < E / 2; ++e) v[e] = (EXACT || t + T * e < nin) ? dr[dLine * (t + T * e)] : make_double2(0.0, 0.0);
#pragma unroll
            for (int e = E / 2; e < E; ++e) v[e] = make_double2(0.0, 0.0);
            fwd(v);
            if constexpr (ZE) {
                cplx* stage = reinterpret_cast<cplx*>(smem);
                if constexpr (forward_ends_local<C, LL>()) LSFC_BARRIER();   // other waves may still read the exchange buffer
#pragma unroll
                for (int e = 0; e < H; ++e) stage[(t + T * e) * LINES + li] = sv[e];
                if (t == 0) stage[(C::L / 2) * LINES + li] = smid;
                LSFC_BARRIER();
#pragma unroll
                for (int e = 0; e < H; ++e) {
                    v[e] = cmul(v[e], sv[e]);
                    v[e + H] = cmul(v[e + H], stage[part[e] * LINES + li]);
                }
                LSFC_BARRIER();
            } else {
#pragma unroll
                for (int e = 0; e < E; ++e) v[e] = cmul(v[e], sv[e]);
            }
            inv(v);
#pragma unroll
            for (int e = 0; e < E / 2; ++e) if (EXACT || t + T * e < nin) dr[dLine * (t + T * e)] = v[e];
            // (every exchange ends with a barrier after its reads: the buffer is free for the next member)
        }
        return;
    }
#pragma unroll
    for (int e = 0; e < E / 2; ++e) v[e] = (EXACT || t + T * e < nin) ? d[dLine * (t + T * e)] : make_double2(0.0, 0.0);
#pragma unroll
    for (int e = E / 2; e < E; ++e) v[e] = make_double2(0.0, 0.0);
    if constexpr (ZE) {
        constexpr int H = E / 2;
        int part[H];
#pragma unroll
        for (int e = 0; e < H; ++e) part[e] = zm[t + T * e];
        cplx sv[H];
        if constexpr (PREFETCH) {
#pragma unroll
            for (int e = 0; e < H; ++e) sv[e] = s[sLine * (t + T * e)];
        }
        fwd(v);
        if constexpr (!PREFETCH) {
#pragma unroll
            for (int e = 0; e < H; ++e) sv[e] = s[sLine * (t + T * e)];
        }
        // stage this line's stored half in LDS (the exchange buffer is free between the two transforms)
        cplx* stage = reinterpret_cast<cplx*>(smem);
        if constexpr (forward_ends_local<C, LL>()) LSFC_BARRIER();   // other waves may still read the exchange buffer
#pragma unroll
        for (int e = 0; e < H; ++e) stage[(t + T * e) * LINES + li] = sv[e];
        if (t == 0) stage[(C::L / 2) * LINES + li] = s[sLine * (C::L / 2)];
        LSFC_BARRIER();
#pragma unroll
        for (int e = 0; e < H; ++e) {
            v[e] = cmul(v[e], sv[e]);
            v[e + H] = cmul(v[e + H], stage[part[e] * LINES + li]);
        }
        LSFC_BARRIER();
    } else if constexpr (PREFETCH) {
        // issue the symbol loads before the forward transform: their HBM latency hides behind its butterflies
        cplx sv[E];
#pragma unroll
        for (int e = 0; e < E; ++e) sv[e] = s[sLine * (t + T * e)];
        fwd(v);
#pragma unroll
        for (int e = 0; e < E; ++e) v[e] = cmul(v[e], sv[e]);
    } else {
        fwd(v);
#pragma unroll
        for (int e = 0; e < E; ++e) v[e] = cmul(v[e], s[sLine * (t + T * e)]);
    }
    inv(v);
#pragma unroll
    for (int e = 0; e < E / 2; ++e) if (EXACT || t + T * e < nin) d[dLine * (t + T * e)] = v[e];
}

// the XCD this wave runs on (HW_REG_XCC_ID, bits 3:0)
__device__ __forceinline__ unsigned xcc_id() {
    unsigned v;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(v));
    return v & 7u;
}
// opaque copy of a value: the optimiser may not carry anything derived from the original across this point (used to keep
// loop-invariant address arithmetic from being hoisted into registers that then live across the whole tile loop)
template <class V> __device__ __forceinline__ V launder_v(V x) { asm volatile("" : "+v"(x)); return x; }
template <class P> __device__ __forceinline__ P launder_s(P x) { asm volatile("" : "+s"(x)); return x; }

// Persistent, software-pipelined form of the fused pass (z-even symbol, 8-line tiles of the 3D layout).
// Why: with one workgroup per CU (the exchange buffer of a 1024-point tile fills the LDS) the plain kernel runs its
// memory phases and its compute phases one after the other -- SQ counters at 512^3: waves parked 36 % of their life,
// VALU active 21 %, and a CU cannot pull its 161 KB per tile faster than ~24 GB/s (6.7 us of the 11.2 us per tile).
// Here one workgroup per CU walks over tiles b, b + G, b + 2G, ... and keeps the NEXT tile's data loads in flight under
// the inverse transform of the current tile (they re-use the registers of the symbol values, which are dead after the
// multiply), the symbol loads in flight under the forward transform as before, and the stores of the previous tile
// drain under the next forward transform.  The stage-twiddle table and the mirror-slot table are set up once per
// workgroup instead of once per tile.  Register pressure is that of the plain PREFETCH variant.
// HALF: 4-line workgroups on half tiles (as k_zfused's HALF), TWO per CU: the exchange buffer of a whole 1024-point tile leaves
// room for one workgroup only, whose eight waves then march in lock step through VALU phases and LDS phases that never
// overlap (SQ counters at 512^3: 2.1 ms of VALU issue per SIMD + 2.2 ms of LDS array time inside a 5.3 ms pass).  Two
// independent half-tile workgroups drift apart and fill each other's phases.  The two halves of a tile (64 B each of every
// 128-B line) must pass through the same L2 at about the same time or every line is fetched twice; a static walk does
// not hold that over hundreds of tiles (measured: 29 GB read instead of 17), so the work is handed out per XCD: tickets
// c = 0, 1, 2, ... from tickets[xcd] (one atomic per workgroup and tile, fetched a whole forward transform before it is
// needed) mean the halves of tiles xcd-th pair of each group of 8 pairs (see `locate`), so the halves of a tile -- and the
// tile of the mirror row, which reads the same symbol rows -- go to the next workgroups of that XCD that become free.  A workgroup whose queue is exhausted moves on to the next queue (xcd + 1, ...), so every ticket of
// every queue is drawn whatever the placement of the workgroups (and the tail balances itself); it ends when all eight
// are exhausted.  There is no waiting on other workgroups anywhere.
// the exchange buffer, which between the transforms also stages the symbol's (L / 2 + 1) x LINES whole-complex mirror values
template <class C, int LINES, bool SPLIT, bool HALF> constexpr size_t persist_xbuf_bytes() {
    using LL = LdsLayout<LINES, HALF ? -1 : 3, SPLIT>;
    constexpr size_t ex = (size_t)LL::line_elems(C::L) * LINES * LL::elem_bytes(), stg = (size_t)(C::L / 2 + 1) * LINES * sizeof(cplx);
    return ex > stg ? ex : stg;
}
template <class C, int LINES, bool SPLIT, bool TWL, bool HALF> constexpr size_t persist_lds_bytes() {
    return persist_xbuf_bytes<C, LINES, SPLIT, HALF>() + (TWL ? (size_t)C::TWLEN * sizeof(cplx) : 0);
}
// workgroups per CU a persistent kernel is bounded for: two half-tile workgroups where the LDS holds them (one definition for the
// kernel's launch bounds and for PassForm::wpe)
template <class C, int LINES, bool SPLIT, bool TWL, bool HALF> constexpr int persist_wpe() {
    return (HALF && 2 * persist_lds_bytes<C, LINES, SPLIT, TWL, HALF>() <= (size_t)160 * 1024) ? 2 : 1;
}
// TICKETS without HALF: whole tiles handed out the same way, in pairs (row, mirror row) per XCD queue.
// XL (round 3) is a set of bits, chosen by the run-time knob "xlane" (0, 1, 3, 5; -1 = 5 where available, else 1):
// XL & 1: the exchange between the two radix-8 stages of the line runs through the lanes of the wavefront (fft_core.hpp:
// xlane_transpose8) instead of LDS -- one LDS exchange and two workgroup barriers less per direction (-0.28 ms at 512^3).
// XL & 4: work items are row PAIRS whose shared symbol values stay in registers (see PAIR below; -0.05 ms).
// XL & 2 (measured slower, kept for A/B runs): in addition the mirror values of the z-even symbol (slots e >= E/2: the entry of frequency L - kz) are loaded by the
// thread that needs them, a second read of lines this workgroup fetches anyway (L2 hits), instead of being staged through
// LDS by the threads that hold them: 8 ds_write_b128 + 8 ds_read_b128 per thread and one of the two barriers around them go.
template <class C, int LINES, bool SPLIT, bool EXACT, bool TWL, bool LATE_SYM = false, bool HALF = false, bool TICKETS = HALF, int XL = 0>
__global__ __launch_bounds__(C::T * LINES, (persist_wpe<C, LINES, SPLIT, TWL, HALF>()))
void k_zfused_persist(cplx* __restrict__ data, const cplx* __restrict__ sym, const cplx* __restrict__ tw,
                      int nouter, int64_t dGrp, int64_t dOuter, int64_t dLine, int64_t sGrp, int64_t sOuter, int64_t sLine,
                      const int2* __restrict__ ytab, const int* __restrict__ zm, int nin, unsigned ntiles, unsigned* __restrict__ tickets) {
    using LL = LdsLayout<LINES, HALF ? -1 : 3, SPLIT>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int T = C::T, E = C::E, H = E / 2;
#ifdef LSFC_NO_STAGE_STORES
    constexpr bool WS = false;
#else
    constexpr bool WS = true;                           // exchange stores from inside the stages (fft_core.hpp: stage<..., LLW>)
#endif
    // ... with the buffer-freeing barriers taken inside the next stage, before its first store (BARF), instead of right after the
    // loads: measured SLOWER (same-box A/B 4.88 -> 5.06 ms: the barrier then separates a wave's butterflies from its own stores);
    // off, kept for A/B builds (make EXTRA=-DLSFC_DEFERRED_BARRIERS)
#ifdef LSFC_DEFERRED_BARRIERS
    constexpr bool DEFER = true;
#else
    constexpr bool DEFER = false;
#endif
    const int li = threadIdx.x % LINES, t = threadIdx.x / LINES;
    // XL & 4 (PAIR; ticketed whole tiles): a work item is a row pair -- the tile of a row and of its mirror row, which multiply by the
    // same symbol values -- and the workgroup runs the two tiles back to back with ONE load of those values: they stay in registers
    // across the first tile's inverse transform and the second tile's forward transform (8 of the 24 loads of every second tile go)
    constexpr bool PAIR = (XL & 4) != 0 && TICKETS && !HALF;
    // work item: a tile (static walk b, b + G, ...) or, HALF, a ticket of this workgroup's XCD
    // (HALF: a work item is (ticket << 3 | queue); DONE = nothing left anywhere)
    constexpr unsigned DONE = 0xFFFFFFFFu;
    unsigned cur = blockIdx.x, nwork = ntiles;
    unsigned* slot = nullptr;                           // HALF: where thread 0 publishes the work item it drew
    unsigned queue = 0, queues_left = 8;                // HALF, thread 0: the queue it draws from, queues not yet seen empty
    [[maybe_unused]] unsigned parity = 1u;              // XL = 2: which of the two ticket slots the next publication uses (slot[0]: the first draw)
    auto draw = [&]() -> unsigned {                     // (thread 0 only)
        while (queues_left > 0) {
            const unsigned c = atomicAdd(tickets + queue, 1u);
            if (c < nwork) return (c << 3) | queue;
            queue = (queue + 1) & 7u; --queues_left;
        }
        return DONE;
    };
    if constexpr (TICKETS) {
        queue = xcc_id();
        nwork = HALF ? ntiles / 4 : (PAIR ? ntiles / 16 : ntiles / 8);   // (ntiles / 8 tiles per queue) [x 2 halves | as pairs]; the host checks ntiles % 16 == 0
        slot = reinterpret_cast<unsigned*>(smem + persist_lds_bytes<C, LINES, SPLIT, TWL, HALF>());
        if (threadIdx.x == 0) *slot = draw();
        __syncthreads();
        cur = __builtin_amdgcn_readfirstlane(*slot);
        __syncthreads();
        if (cur == DONE) return;
    } else if (cur >= nwork) return;                    // (uniform per workgroup; no inter-workgroup synchronisation anywhere)
    if constexpr (TWL) {
        cplx* tl = reinterpret_cast<cplx*>(smem + persist_xbuf_bytes<C, LINES, SPLIT, HALF>());
        for (int i = threadIdx.x; i < C::TWLEN; i += C::T * LINES) tl[i] = tw[i];
        __syncthreads();
        tw = tl;
    }
    // Addressing: a tile's base addresses are uniform (scalar registers), the thread's part is one 32-bit offset --
    // 64-bit per-thread pointers kept across the loop cost the registers that decide between "fits" and "spills", and a
    // spill reload at the loop top would make the wave wait for the previous tile's stores (scratch and global memory
    // share the in-order vmcnt counter).
    auto locate = [&](unsigned w, cplx*& dbase, const cplx*& sbase, unsigned sub = 0) {
        unsigned tl_ = w; int half = 0;
        // (ticket -> tile, half: fft_core.hpp ticket_decode)
        if constexpr (PAIR) tl_ = ticket_decode_pair(w, sub);
        else if constexpr (TICKETS) { unsigned hf; ticket_decode<HALF>(w, tl_, hf); half = (int)hf * LINES; }
        const int o = (int)(tl_ % (unsigned)nouter), g = (int)(tl_ / (unsigned)nouter);
        int outer = o, srow = o;
        if (ytab) { const int2 e2 = ytab[o]; outer = e2.x; srow = e2.y; }
        dbase = data + g * dGrp + outer * dOuter + half;
        sbase = sym + g * sGrp + srow * sOuter + half;
    };
    // (unsigned: scalar base + zero-extended 32-bit lane offset is an addressing mode of the global instructions)
    const unsigned doff = (unsigned)(li + (int)dLine * t), dstep = (unsigned)((int)dLine * T);      // element j = t + T e of this thread's line
    const unsigned soff = (unsigned)(li + (int)sLine * t), sstep = (unsigned)((int)sLine * T);
    // (tried in round 3: the uniform part dstep * e of an element index moved into the scalar base, (base + dstep * e)[doff] -- one
    // lane offset instead of a per-lane add per element: neutral at 1024 points, slower on the 768-point line; not kept)
    constexpr bool MIRG = (XL & 2) != 0;
    [[maybe_unused]] unsigned moff[MIRG ? H : 1];      // MIRG: element index of the mirror entry of slot e + H in this thread's symbol line
    if constexpr (MIRG) {
#pragma unroll
        for (int e = 0; e < H; ++e) moff[e] = (unsigned)(li + (int)sLine * zm[t + T * e]);
    }
    cplx nd[H];                                        // data of the tile about to be transformed
    {
        cplx* d; const cplx* s;
        locate(cur, d, s);
#pragma unroll
        for (int e = 0; e < H; ++e) nd[e] = (EXACT || t + T * e < nin) ? d[doff + dstep * e] : make_double2(0.0, 0.0);
    }
    [[maybe_unused]] unsigned sub = 0;                  // PAIR: which tile of the pair `cur` is being processed
    [[maybe_unused]] const cplx* sheld = nullptr;       // PAIR: the symbol tile whose values sv_pair / smid_pair hold
    [[maybe_unused]] cplx sv_pair[PAIR ? H : 1];        // PAIR: the symbol values live across the two tiles of a pair (loop-carried registers)
    [[maybe_unused]] cplx smid_pair = make_double2(0.0, 0.0);
    for (;;) {
        // HALF: draw the next ticket now; it is published and read around the barriers of the symbol multiply below
        unsigned drawn = 0;
        if constexpr (TICKETS) { if (threadIdx.x == 0 && (!PAIR || sub == 0)) drawn = draw(); }
        cplx v[E];
#pragma unroll
        for (int e = 0; e < H; ++e) { v[e] = nd[e]; v[e + H] = make_double2(0.0, 0.0); }
        cplx sv_tile[PAIR ? 1 : H];
        cplx (&sv)[H] = *reinterpret_cast<cplx (*)[H]>(PAIR ? &sv_pair[0] : &sv_tile[0]);
        [[maybe_unused]] cplx smr[MIRG ? H : 1];
        cplx smid_tile = make_double2(0.0, 0.0);
        cplx& smid = PAIR ? smid_pair : smid_tile;
        auto load_symbol = [&] {
            cplx* d; const cplx* s;
            locate(cur, d, s, sub);
            if constexpr (PAIR) {
                if (s == sheld) return;                 // (uniform) the mirror row's tile: same symbol values, already in registers
                sheld = s;
            }
            const unsigned so = launder_v(soff);
#pragma unroll
            for (int e = 0; e < H; ++e) sv[e] = s[so + sstep * e];
            if constexpr (MIRG) {
#pragma unroll
                for (int e = 0; e < H; ++e) smr[e] = s[moff[e]];
            } else {
                if (t == 0) smid = s[so - (unsigned)((int)sLine * t) + (unsigned)((int)sLine * (C::L / 2))];
            }
        };
        if constexpr (!SPLIT && WS) {
            // exchange stores issued from inside the stages (fft_forward_ws); the symbol is loaded after the first stage
            if constexpr (!LATE_SYM) load_symbol();
            fft_forward_ws<C, LL, true, TWL, DEFER, (XL > 0)>(v, t, tw, smem, 0, li, [&] { if constexpr (LATE_SYM) load_symbol(); });
        } else if constexpr (LATE_SYM) {
            // the first forward stage (the widest butterfly plus its twiddles) runs before the symbol values occupy registers
            stage<C, 0, +1, 1, TWL>(v, t, tw);
            load_symbol();
            exchange<C, 0, 1, LL>(v, t, smem, 0, li);
            stage<C, 1, +1, 0, TWL>(v, t, tw);
            if constexpr (C::NS >= 3) { exchange<C, 1, 2, LL>(v, t, smem, 0, li); stage<C, 2, +1, 0, TWL>(v, t, tw); }
            if constexpr (C::NS >= 4) { exchange<C, 2, 3, LL>(v, t, smem, 0, li); stage<C, 3, +1, 0, TWL>(v, t, tw); }
        } else {
            load_symbol();
            fft_forward<C, LL, true, TWL>(v, t, tw, smem, 0, li);
        }
        cplx* stage = reinterpret_cast<cplx*>(smem);
        unsigned next = cur + gridDim.x;
        if constexpr (MIRG) {
            // no staging: every thread holds its own mirror values.  The ticket travels through a slot of its own per tile parity,
            // so ONE barrier publishes it (the slot of the other parity is rewritten only two barriers later)
#pragma unroll
            for (int e = 0; e < H; ++e) { v[e] = cmul(v[e], sv[e]); v[e + H] = cmul(v[e + H], smr[e]); }
            if constexpr (TICKETS) {
                if (threadIdx.x == 0) slot[parity] = drawn;
                LSFC_BARRIER();
                next = __builtin_amdgcn_readfirstlane(slot[parity]);
                parity ^= 1u;
            }
        } else {
        // other waves may still read the exchange buffer (wave-local last exchange, or the deferred barrier of fft_forward_ws)
        if constexpr (forward_ends_local<C, LL>() || (!SPLIT && WS && DEFER)) LSFC_BARRIER();
#pragma unroll
        for (int e = 0; e < H; ++e) stage[(t + T * e) * LINES + li] = sv[e];
        if (t == 0) stage[(C::L / 2) * LINES + li] = smid;
        if constexpr (TICKETS) { if (threadIdx.x == 0 && (!PAIR || sub == 0)) *slot = drawn; }
        LSFC_BARRIER();
        {
            const int* zmt = launder_s(zm) + t;            // (re-read per tile from L1: eight registers less across the loop)
#pragma unroll
            for (int e = 0; e < H; ++e) {
                v[e] = cmul(v[e], sv[e]);
                v[e + H] = cmul(v[e + H], stage[zmt[T * e] * LINES + li]);
            }
        }
        // next tile: its loads travel while this tile is transformed back
        if constexpr (TICKETS) next = __builtin_amdgcn_readfirstlane(*slot);
        LSFC_BARRIER();
        }
        // PAIR: after the first tile of a pair comes its second; the drawn ticket (in the slot since the first tile) is for afterwards
        const bool more = PAIR ? (sub == 0 || next != DONE) : (TICKETS ? next != DONE : next < nwork);
        if (more) {
            cplx* dn; const cplx* sn;
            if (PAIR && sub == 0) locate(cur, dn, sn, 1u); else locate(next, dn, sn, 0u);
            const unsigned dof = launder_v(doff);
#pragma unroll
            for (int e = 0; e < H; ++e) nd[e] = (EXACT || t + T * e < nin) ? dn[dof + dstep * e] : make_double2(0.0, 0.0);
        }
        if constexpr (!SPLIT && WS) fft_inverse_ws<C, LL, true, TWL, DEFER, (XL > 0)>(v, t, tw, smem, 0, li);
        else fft_inverse<C, LL, true, TWL>(v, t, tw, smem, 0, li);
        {
            cplx* d; const cplx* s;
            locate(cur, d, s, sub);
            const unsigned dof = launder_v(doff);
#pragma unroll
            for (int e = 0; e < H; ++e) if (EXACT || t + T * e < nin) d[dof + dstep * e] = v[e];
        }
        if (!more) break;
        if constexpr (PAIR) { if (sub == 0) sub = 1; else { sub = 0; cur = next; } }
        else cur = next;
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// opt a kernel in to > 48 KiB of dynamic LDS, once per kernel and device (not on every launch)
template <class K> static void allow_lds(K kernel, size_t bytes) {
    if (bytes <= 48 * 1024) return;
    static std::mutex mu;
    static std::set<std::pair<const void*, int>> done;
    int dev = 0; LSFC_HIP(hipGetDevice(&dev));
    const std::pair<const void*, int> key(reinterpret_cast<const void*>(kernel), dev);
    std::lock_guard<std::mutex> lock(mu);
    if (done.count(key)) return;
    LSFC_HIP(hipFuncSetAttribute(key.first, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    done.insert(key);
}

// developer switches read once per process (the launch paths run per apply)
static bool env_flag_no_sibling_pairs() { static const bool v = getenv("LSFC_NO_SIBLING_PAIRS") != nullptr; return v; }
static bool env_flag_z_quarter() { static const bool v = [] { const char* e = getenv("LSFC_Z_QUARTER"); return e && e[0] == '1'; }(); return v; }

template <class C> struct Tune {
    // lines per workgroup: contiguous passes use 256-thread workgroups; strided passes
    // interleave XB lines unless that would exceed 512 threads.
    static constexpr int LPW = (256 / C::T) > 0 ? (256 / C::T) : 1;
    static constexpr int LINES = (C::T * XB <= 512 || (C::E <= 8 && C::T * XB <= 1024)) ? XB : 512 / C::T;
    // the y passes (no symbol, no second transform) of the 2048-point line: whole 128-B chunks from 1024-thread workgroups
    // (16 waves, 128 registers each; split exchanges: 147 KB of LDS) instead of 64-B half chunks from 512 threads
#ifdef LSFC_Y2048_HALF
    static constexpr int YLINES = LINES;
#else
    static constexpr int YLINES = (C::L == 2048 && C::T * XB <= 1024) ? XB : LINES;
#endif
};

// The lines of this family, and the way from a run-time line length to its Cfg: f(C{})
template <class... C> struct Lines {};
#if LSFC_FAMILY == 2
using FamilyLines = Lines<Cfg32, Cfg64, Cfg128, Cfg256, Cfg512, Cfg1024, Cfg2048>;
#elif LSFC_FAMILY == 3
using FamilyLines = Lines<Cfg48, Cfg96, Cfg192, Cfg384, Cfg768, Cfg1536>;
#else
using FamilyLines = Lines<Cfg80, Cfg160, Cfg320, Cfg640, Cfg1280>;
#endif
template <class... C, class F> static void dispatch_line(Lines<C...>, int L, F&& f) {
    if (!((L == C::L && (f(C{}), true)) || ...)) fail(LSFC_EINVAL, "pruned pipeline: unsupported padded length %d", L);
}
template <class F> static void dispatch_line(int L, F&& f) { dispatch_line(FamilyLines{}, L, f); }

// the two x passes: INV = false xfwd, true xinv
template <bool INV, class C, bool SPLIT, bool FULL> static void xpass_t(const XPass& a, int wmagic, int64_t bstride, hipStream_t st) {
    constexpr int LPW = Tune<C>::LPW;
    using LL = LdsLayout<1, 3, SPLIT>;
    const size_t lds = (size_t)LL::line_elems(C::L) * LPW * LL::elem_bytes();
    const dim3 grid((unsigned)((a.nlines + LPW - 1) / LPW), (unsigned)a.nrhs), block(C::T * LPW);
    auto launch = [&](auto k, auto... args) { allow_lds(k, lds); hipLaunchKernelGGL(k, grid, block, lds, st, args...); };
    // a complex nu (nu.im): the kernel of the same form that multiplies by both planes
    if constexpr (INV) {
        if (a.nu.im) launch(k_xinv_c<C, LPW, SPLIT, FULL>, (const cplx*)a.work, a.vb, a.wbatch, a.alpha, a.beta, a.tw, a.nlines, wmagic, a.W, a.Wp, a.n, bstride, a.nu.re, a.nu.im, (int)a.conj);
        else launch(k_xinv<C, LPW, SPLIT, FULL>, (const cplx*)a.work, a.vb, a.wbatch, a.alpha, a.beta, a.tw, a.nlines, wmagic, a.W, a.Wp, a.n, bstride, a.nu.re, (int)a.conj);
    } else {
        if (a.nu.im) launch(k_xfwd_c<C, LPW, SPLIT, FULL>, a.vb, a.wbatch, a.nu.re, a.nu.im, a.work, a.tw, a.nlines, wmagic, a.W, a.Wp, a.n, bstride, (int)a.conj);
        else launch(k_xfwd<C, LPW, SPLIT, FULL>, a.vb, a.wbatch, a.nu.re, a.work, a.tw, a.nlines, wmagic, a.W, a.Wp, a.n, bstride, (int)a.conj);
    }
}
static void ytile(const PrunedTuning& tn, int L, int ngrp, int l, int& TG, int& TZ) {
    // auto (0): all groups x 1 plane, except at L >= 1024 where 32 groups x 8 planes keeps the 128-B chunks that the
    // workgroups in flight touch together within a few DRAM pages / TLB entries of both arrays (yinv 3.3 -> 2.8 ms)
    const int ag = (L >= 1024) ? 32 : ngrp, az = (L >= 1024) ? 8 : 1;
    TG = tn.ytile_g > 0 ? tn.ytile_g : ag; if (TG > ngrp) TG = ngrp; while (ngrp % TG) --TG;
    TZ = tn.ytile_z > 0 ? tn.ytile_z : az; if (TZ > l) TZ = l;       while (l % TZ) --TZ;
}
// the two y passes: INV = false yfwd (a1 -> a2), true yinv (a2 -> a1)
template <bool INV, class C, bool SPLIT, int WPE, bool FULL> static void ypass_t(const PassForm& f, const YPass& a, hipStream_t st) {
    constexpr int LINES = Tune<C>::YLINES;
    using LL = LdsLayout<LINES, 3, SPLIT>;
    const size_t lds = (size_t)LL::line_elems(C::L) * LINES * LL::elem_bytes();
    auto k = INV ? k_yinv<C, LINES, SPLIT, WPE, FULL> : k_yfwd<C, LINES, SPLIT, WPE, FULL>;
    allow_lds(k, lds);
    hipLaunchKernelGGL(k, dim3((unsigned)((a.Lx / LINES) * a.l), (unsigned)a.nrhs), dim3(C::T * LINES), lds, st, (const cplx*)(INV ? a.a2 : a.a1), INV ? a.a1 : a.a2,
                       a.tw, a.Lx, a.m, a.l, f.tg, f.tz, a.p1, a.p2, a.batch1, a.batch2);
}
template <class C, bool SPLIT, bool PREFETCH, int WPE, bool ZE> static void zfused_t(const PassForm& f, const FusedPass& a, hipStream_t st) {
    const FusedGeom& g = a.g;
    // g.dTile / g.sTile are strides per XB-tile of x'; a workgroup covers LINES of the XB lines of a tile.
    // twl != NULL: full stage-twiddle table, staged in LDS by the kernel.
    constexpr int LINES = Tune<C>::LINES;
    static_assert(XB % LINES == 0, "LINES must divide XB");
    using LL = LdsLayout<LINES, 3, SPLIT>;
    size_t lds = (size_t)LL::line_elems(C::L) * LINES * LL::elem_bytes();
    const cplx* twl = f.twl ? a.twl : nullptr;  // (switched off, or the table does not fit beside the exchange buffer: z_form)
    const cplx* tw = twl ? twl : a.tw;
    if (twl) lds += (size_t)C::TWLEN * sizeof(cplx);
    decltype(&k_zfused<C, LINES, SPLIT, PREFETCH, WPE, false, ZE, false, false>) k = nullptr;
    dispatch_flags({f.full, twl != nullptr, f.batch}, [&](auto FULL, auto TWL, auto BATCH) {
        // batch: one symbol load per tile for all right-hand sides (the symbol is always loaded up front there, so the
        // PREFETCH flavours share one instantiation)
        k = k_zfused<C, LINES, SPLIT, PREFETCH && !BATCH, WPE, false, ZE, FULL, TWL, BATCH>;
    });
    allow_lds(k, lds);
    if (LINES == XB) {
        hipLaunchKernelGGL(k, dim3((unsigned)((g.Lx / XB) * g.nouter)), dim3(C::T * LINES), lds, st, a.data, a.sym, tw, g.nouter,
                           g.dTile, g.dOuter, g.dLine, g.sTile, g.sOuter, g.sLine, g.ytab, g.zm, g.nin, a.nrhs, a.dBatch,
                           // (pairing a row with its mirror row on one XCD here too -- blocks b and b + 8 -- measured neutral on the
                           // one-tile and the multi-right-hand-side forms at 48^3 ... 256^3: left off)
                           0);
    } else {
        // split each tile into XB/LINES sub-groups: sub-group h starts at xi offset h*LINES
        // (tile, sub-group) collapse to one group index only when tiles are XB-contiguous in xi (2D natural layout)
        LSFC_REQUIRE(g.dTile == XB && g.sTile == XB, "sub-tile groups need the natural (2D) layout");
        hipLaunchKernelGGL(k, dim3((unsigned)((g.Lx / LINES) * g.nouter)), dim3(C::T * LINES), lds, st, a.data, a.sym, tw, g.nouter,
                           (int64_t)LINES, g.dOuter, g.dLine, (int64_t)LINES, g.sOuter, g.sLine, g.ytab, g.zm, g.nin, a.nrhs, a.dBatch,
                           (XB / LINES == 2 && g.nouter == 1 && (g.Lx / LINES) % 16 == 0 && !env_flag_no_sibling_pairs()) ? 1 : 0);
    }
}

// persistent pipelined fused pass: z-even symbol, whole 8-line tiles (3D layout); one workgroup per CU
static int cu_count() {
    static int cus = 0;
    if (!cus) { int dev = 0; LSFC_HIP(hipGetDevice(&dev)); hipDeviceProp_t pr; LSFC_HIP(hipGetDeviceProperties(&pr, dev)); cus = pr.multiProcessorCount > 0 ? pr.multiProcessorCount : 256; }
    return cus;
}
static unsigned* ticket_set(hipStream_t st);
template <class C, bool SPLIT, bool LATE_SYM, bool TICKETS> static void zfused_persist_t(const PassForm& f, const FusedPass& a, hipStream_t st) {
    const FusedGeom& g = a.g;
    constexpr int LINES = XB;
    using LL = LdsLayout<LINES, 3, SPLIT>;
    size_t lds = persist_xbuf_bytes<C, LINES, SPLIT, false>();
    const cplx* twl = f.twl ? a.twl : nullptr;
    const cplx* tw = twl ? twl : a.tw;
    if (twl) lds += (size_t)C::TWLEN * sizeof(cplx);
    const int xl = f.xl;                     // resolved by z_form: 0, 1, and with the table 3 or (ticketed) 5
    // lane exchanges between stages of equal radix (whole-complex whole tiles, symbol after the first stage: the 512^3 and 256^3 forms)
    constexpr bool XLANE = xlane_ok<C, LL>() && !SPLIT && LATE_SYM;
    decltype(&k_zfused_persist<C, LINES, SPLIT, false, false, LATE_SYM, false, TICKETS>) k = nullptr;
    dispatch_flags({f.full, twl != nullptr}, [&](auto FULL, auto TWL) {
        if (xl == 0) k = k_zfused_persist<C, LINES, SPLIT, FULL, TWL, LATE_SYM, false, TICKETS>;
        else if constexpr (!XLANE) fail(LSFC_EINVAL, "internal: lane exchanges requested from a persistent form that has none");
        else if (xl == 1) k = k_zfused_persist<C, LINES, SPLIT, FULL, TWL, LATE_SYM, false, TICKETS, 1>;
        // 3: + mirror symbol values from L2 (XL & 2; measured slower, profiles/r03_experiment_fused_pass_variants.log)
        else if constexpr (!TWL) fail(LSFC_EINVAL, "internal: persistent fused pass with lane-exchange form %d", xl);
        else if (xl == 5 && TICKETS) k = k_zfused_persist<C, LINES, SPLIT, FULL, TWL, LATE_SYM, false, TICKETS, 5>;
        else if (xl == 3) k = k_zfused_persist<C, LINES, SPLIT, FULL, TWL, LATE_SYM, false, TICKETS, 3>;
        else fail(LSFC_EINVAL, "internal: persistent fused pass with lane-exchange form %d", xl);
    });
    if (TICKETS) lds += 16;                             // the ticket slots
    allow_lds(k, lds);
    const int cus = cu_count();
    const unsigned ntiles = (unsigned)((g.Lx / XB) * g.nouter);
    // workgroups per CU that fit (LDS-limited); the walk stays interleaved so that co-resident workgroups touch neighbouring tiles
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(4, ((size_t)160 * 1024) / lds));
    const unsigned grid = std::min<unsigned>(ntiles, (unsigned)(cus * per_cu));
    hipLaunchKernelGGL(k, dim3(grid), dim3(C::T * LINES), lds, st, a.data, a.sym, tw, g.nouter,
                       g.dTile, g.dOuter, g.dLine, g.sTile, g.sOuter, g.sLine, g.ytab, g.zm, g.nin, ntiles, TICKETS ? ticket_set(st) : (unsigned*)nullptr);
}
// Ticket counters of the half-tile pass: 8 (one per XCD) per launch, zeroed on the launch's stream just before it.  A ring of
// 64 sets per device, so that launches in flight on different streams (chunks of a distributed plan) never share a set.
static unsigned* ticket_set(hipStream_t st) {
    static std::mutex mu;
    static std::map<int, std::pair<unsigned*, unsigned>> ring;
    int dev = 0; LSFC_HIP(hipGetDevice(&dev));
    unsigned* base; unsigned idx;
    {
        std::lock_guard<std::mutex> lock(mu);
        auto it = ring.find(dev);
        if (it == ring.end()) {
            unsigned* p = nullptr;
            LSFC_HIP(hipMalloc(&p, 64 * 8 * sizeof(unsigned)));
            it = ring.emplace(dev, std::make_pair(p, 0u)).first;
        }
        base = it->second.first; idx = it->second.second++ % 64u;
    }
    unsigned* set = base + 8 * idx;
    LSFC_HIP(hipMemsetAsync(set, 0, 8 * sizeof(unsigned), st));
    return set;
}
// the same on half tiles: 4-line workgroups with the twiddle table, as many per CU as the LDS holds (two at L = 1024)
template <class C> static void zfused_persist_half_t(const PassForm& f, const FusedPass& a, hipStream_t st) {
    const FusedGeom& g = a.g;
    if constexpr (C::L >= 1024) {
        constexpr int LINES = XB / 2;
        constexpr size_t lds = persist_lds_bytes<C, LINES, false, true, true>() + 16;   // + the ticket slot
        static_assert(lds <= (size_t)160 * 1024, "half-tile persistent pass: exchange buffer exceeds the LDS");
        constexpr bool XLANE = xlane_ok<C, LdsLayout<LINES, -1, false>>();
        decltype(&k_zfused_persist<C, LINES, false, false, true, true, true>) k = nullptr;
        dispatch_flags({f.full, XLANE && f.xl != 0}, [&](auto FULL, auto XL) {
            if constexpr (XLANE || !XL) k = k_zfused_persist<C, LINES, false, FULL, true, true, true, true, XL ? 1 : 0>;
        });
        // (tried in round 3: the ONE LDS exchange left per direction run split -- real parts, then imaginary parts, through half the
        // buffer -- so that TWO half-tile workgroups fit a CU at 1280 / 1536 points: without the in-stage stores every output of the
        // widest butterfly stays live next to the symbol values in flight, the kernels spill (240 / 472 bytes per lane), 640^3 ties
        // at 30.4 ms and 768^3 loses 49.3 -> 60.7 ms; removed, profiles/r03_experiment_lane_exchange_radix4.log)
        LSFC_REQUIRE(a.twl != nullptr, "half-tile persistent pass: twiddle table missing");
        allow_lds(k, lds);
        const unsigned ntiles = (unsigned)((g.Lx / XB) * g.nouter);
        LSFC_REQUIRE(ntiles % 16 == 0 && (g.nouter % 2 == 0 || !g.ytab), "ticketed half-tile z pass needs a multiple of 16 tiles in row pairs");
        const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(2, ((size_t)160 * 1024) / lds));
        const unsigned grid = std::min<unsigned>(2 * ntiles, (unsigned)(cu_count() * per_cu));
        unsigned* tickets = ticket_set(st);
        hipLaunchKernelGGL(k, dim3(grid), dim3(C::T * LINES), lds, st, a.data, a.sym, a.twl, g.nouter,
                           g.dTile, g.dOuter, g.dLine, g.sTile, g.sOuter, g.sLine, g.ytab, g.zm, g.nin, ntiles, tickets);
    } else {
        fail(LSFC_EINVAL, "half-tile persistent pass: lines of %d points run as whole tiles", (int)C::L);
    }
}

// half-tile z pass (L = 1024 and L = 1536 in the 3D tiled layout only): 4-line workgroups, sibling halves 8 blocks apart
// (LINES = 2: quarter tiles -- four sibling workgroups per tile, 32 blocks per group of 8 tiles)
template <class C, bool SPLIT, bool PREFETCH, int WPE, bool ZE, int LINES, bool FULL> static void zfused_half_t(const FusedPass& a, hipStream_t st) {
    const FusedGeom& g = a.g;
    using LL = LdsLayout<LINES, 3, SPLIT>;
    const size_t lds = (size_t)LL::line_elems(C::L) * LINES * LL::elem_bytes();
    auto k = k_zfused<C, LINES, SPLIT, PREFETCH, WPE, true, ZE, FULL, false>;
    allow_lds(k, lds);
    const int64_t ntiles = (int64_t)(g.Lx / XB) * g.nouter;
    LSFC_REQUIRE(ntiles % 8 == 0, "half-tile z pass needs a multiple of 8 tiles");
    hipLaunchKernelGGL(k, dim3((unsigned)((XB / LINES) * ntiles)), dim3(C::T * LINES), lds, st, a.data, a.sym, a.tw, g.nouter,
                       g.dTile, g.dOuter, g.dLine, g.sTile, g.sOuter, g.sLine, g.ytab, g.zm, g.nin, 1, (int64_t)0, 0);
}

// Loads this family's code object (several MB: hundreds of kernel instantiations) on the current device.  HIP loads code
// objects lazily at the first launch from them; done here, once per device at plan creation and followed by a device
// synchronisation, the load never runs concurrently with a caller's transfers or the first real pass.
__global__ void FAM(k_warmup)(int* p) { if (p) *p = 0; }
static void warmup() {
    hipLaunchKernelGGL(FAM(k_warmup), dim3(1), dim3(64), 0, 0, (int*)nullptr);
    LSFC_HIP(hipGetLastError());
}

static void perm(int L, int* freq_of_storage) {
    dispatch_line(L, [&](auto c) { perm_table<decltype(c)>(freq_of_storage); });
}

// ---------------------------------------------------------------------------
// Which kernel a pass runs: pure host functions from what a dispatcher knows (line length, tuning, geometry, number of
// right-hand sides) to a PassForm (pruned.hpp).  The launchers below switch on the PassForm and decide nothing themselves.
// ---------------------------------------------------------------------------
static constexpr size_t LDS_BYTES = (size_t)160 * 1024;
// the compile-time facts of a line length that the choice depends on
struct LineTraits {
    int lines, ylines, twlen;
    size_t tile_lds[2];          // exchange buffer of a one-tile workgroup (`lines` lines): [0] whole complex, [1] split
    size_t persist_lds[2];       // ... of a persistent 8-line workgroup
    size_t xb_full_lds;          // whole-complex exchange of 8 lines
    size_t y_full_lds;           // whole-complex exchange of the y passes' workgroup
    bool xl_tile, xl_half, xl_quarter;   // one-tile kernels: the lane exchange is compiled in (whole-complex exchanges only)
    bool xl_persist;             // persistent whole tiles: lane exchanges available
    bool xl_persist_half;        // ticketed half tiles likewise
    int persist_half_wpe;        // ticketed half tiles: workgroups per CU
};
template <class C> static LineTraits line_traits_t() {
    LineTraits t{};
    constexpr int LINES = Tune<C>::LINES, YLINES = Tune<C>::YLINES;
    t.lines = LINES; t.ylines = YLINES; t.twlen = C::TWLEN;
    t.tile_lds[0] = (size_t)LdsLayout<LINES, 3, false>::line_elems(C::L) * LINES * LdsLayout<LINES, 3, false>::elem_bytes();
    t.tile_lds[1] = (size_t)LdsLayout<LINES, 3, true>::line_elems(C::L) * LINES * LdsLayout<LINES, 3, true>::elem_bytes();
    t.persist_lds[0] = persist_xbuf_bytes<C, XB, false, false>();
    t.persist_lds[1] = persist_xbuf_bytes<C, XB, true, false>();
    t.xb_full_lds = (size_t)LdsLayout<XB, 3, false>::line_elems(C::L) * XB * 16;
    t.y_full_lds = (size_t)LdsLayout<YLINES, 3, false>::line_elems(C::L) * YLINES * 16;
    t.xl_tile = xl_one_tile<C, LINES, false>(); t.xl_half = xl_one_tile<C, 4, false>(); t.xl_quarter = xl_one_tile<C, 2, false>();
    t.xl_persist = xlane_ok<C, LdsLayout<XB, 3, false>>();
    if constexpr (C::L >= 1024) {
        t.xl_persist_half = xlane_ok<C, LdsLayout<XB / 2, -1, false>>();
        t.persist_half_wpe = persist_wpe<C, XB / 2, false, true, true>();
    }
    return t;
}
static LineTraits line_traits(int L) {
    LineTraits t{};
    dispatch_line(L, [&](auto c) { t = line_traits_t<decltype(c)>(); });
    return t;
}

static PassForm xform(PassFamily family, const PrunedTuning& tn, const XPass& a) {
    const int L = a.L, n = a.n;
    PassForm f;
    f.family = family; f.L = L; f.split = tn.split_x; f.full = n == L / 2;
    return f;
}
static PassForm yform(PassFamily family, const PrunedTuning& tn, const YPass& a) {
    const int L = a.L, Lx = a.Lx, m = a.m, l = a.l;
    const LineTraits t = line_traits(L);
    PassForm f;
    f.family = family; f.L = L; f.full = m == L / 2; f.lines = t.ylines;
    // whole-complex exchange buffers of the longest lines exceed the 160 KiB of LDS: those run split whatever split_s says
    f.forced_split = t.y_full_lds > LDS_BYTES;
    f.split = tn.split_s || f.forced_split;
    ytile(tn, L, Lx / t.ylines, l, f.tg, f.tz);
    return f;
}

// chunk addressing of the x passes: s / W by multiplication with wmagic = floor(2^22 / W) + 1 (exact for s < 2048:
// s * (wmagic * W - 2^22) <= s * W < 2^22; the product s * wmagic stays below 2^32 for W >= 2)
static int chunk_magic(int L, int W) {
    LSFC_REQUIRE(W >= 8 && W <= L && L % W == 0 && L <= 2048, "chunk width %d does not divide the line length %d", W, L);
    return (1 << 22) / W + 1;
}
template <bool INV> static void xpass(const PrunedTuning& tn, const XPass& a, hipStream_t st) {
    const int wmagic = chunk_magic(a.L, a.W);
    const int64_t bstride = a.bstride > 0 ? a.bstride : (int64_t)a.Wp * a.nlines;       // dense chunks: [chunk][line][Wp]
    const PassForm f = xform(INV ? PassFamily::XINV : PassFamily::XFWD, tn, a);
    dispatch_line(a.L, [&](auto c) { dispatch_flags({f.split, f.full}, [&](auto SPLIT, auto FULL) {
        xpass_t<INV, decltype(c), SPLIT, FULL>(a, wmagic, bstride, st);
    }); });
    LSFC_HIP(hipGetLastError());
}
template <bool INV> static void ypass(const PrunedTuning& tn, const YPass& a, hipStream_t st) {
    const PassForm f = yform(INV ? PassFamily::YINV : PassFamily::YFWD, tn, a);
    dispatch_line(a.L, [&](auto c) { dispatch_flags({f.split, f.full}, [&](auto SPLIT, auto FULL) {
        ypass_t<INV, decltype(c), SPLIT, 1, FULL>(f, a, st);
    }); });
    LSFC_HIP(hipGetLastError());
}
// (functions of their own, not xpass<false> ... in the table: the table is host code only, and the device pass instantiates the
// kernels of a launcher template only where something it compiles names the launcher)
static void xfwd(const PrunedTuning& tn, const XPass& a, hipStream_t st) { xpass<false>(tn, a, st); }
static void xinv(const PrunedTuning& tn, const XPass& a, hipStream_t st) { xpass<true>(tn, a, st); }
static void yfwd(const PrunedTuning& tn, const YPass& a, hipStream_t st) { ypass<false>(tn, a, st); }
static void yinv(const PrunedTuning& tn, const YPass& a, hipStream_t st) { ypass<true>(tn, a, st); }
static int twfull_len(int L) {
    int len = 0;
    dispatch_line(L, [&](auto c) { len = decltype(c)::TWLEN; });
    return len;
}
static void twfull(int L, const cplx* tw, cplx* out) {
    dispatch_line(L, [&](auto c) { twfull_table<decltype(c)>(out, tw); });
}

// the lane-exchange form a persistent whole-tile kernel runs for the request `req` (knob "xlane")
static int persist_xl(int req, bool available, bool twl, bool tickets) {
    if (!available) return 0;
    if (req == 1) return 1;
    // 3 (+ mirror symbol values from L2) and 5 (+ row pairs as work items, ticketed form only) exist with the twiddle table only;
    // any other request >= 2 runs as 1 with the table, and through LDS without it
    if (req >= 2 && twl) return (req == 5 && tickets) ? 5 : (req == 3 ? 3 : 1);
    return 0;
}
static PassForm zfused_form(const PrunedTuning& tn, const FusedPass& a) {
    const int L = a.L, nrhs = a.nrhs;
    const FusedGeom& g = a.g;
    const bool have_twl = a.twl != nullptr;       // the caller holds the full stage-twiddle table of the line
    const LineTraits t = line_traits(L);
    const int64_t ntiles = (int64_t)(g.Lx / XB) * g.nouter;
    PassForm f;
    f.L = L; f.ze = g.zm != nullptr; f.full = g.nin == L / 2;
    // the half-tile forms (below) take one right-hand side per launch: a batch runs through them member by member
    const bool tiled = g.dLine == 8 && ntiles % 8 == 0;
    // z_half, the flavour of the half-tile one-tile kernels: 0 whole tiles, 1 whole-complex exchange + prefetch, 2 split + prefetch,
    // 3 split, 4 (and above) whole-complex.  auto (-1) at L = 1024: half-tile, split exchanges, symbol prefetch -- 6.95 -> 6.6 ms at
    // 512^3 (profiles/r01_experiment_half_tile.log); with the z-even half symbol the full-tile form wins (6.05 ms,
    // profiles/r01_experiment_even_z.log).  At L = 1536 (24 elements per thread: in 8-line, 512-thread workgroups the fused pass is
    // capped at 256 registers and spills; half tiles, 4 lines, 256 threads, one wave per SIMD, lift the cap) auto is 1
    // (768^3: fused pass 36.7 -> 29.7 ms, apply 64.7 -> 57.4 ms)
    int zh = 0;
    if (LSFC_FAMILY == 2 && L == 1024 && tiled) zh = tn.z_half >= 0 ? tn.z_half : (g.zm ? 0 : 2);
    if (LSFC_FAMILY == 3 && L == 1536 && tiled) zh = tn.z_half >= 0 ? tn.z_half : 1;
    // the 2048-point line in the 3D tiled layout: a whole 8-line tile does not fit the 160 KiB of LDS, half tiles do
    const bool half2048 = LSFC_FAMILY == 2 && L == 2048 && g.dLine == 8;
    const bool half_form = zh > 0 || half2048;
    // persistent pipelined form: z-even symbol, 3D tiled layout, whole 8-line tiles, one right-hand side
    {
        // z_persist: 1 whole-complex exchanges, 2 split exchanges, 3 / 4 the same with the symbol loaded after the first forward
        // stage (its 32 registers stay free during the widest butterfly); auto = 3: 5.24 ms at 512^3 against 5.73 for the
        // one-tile kernel, 0.58 against 0.675 ms at 256^3 (profiles/r02_experiment_persistent_zpass.log)
        // 5: ticketed half tiles.  Auto at L = 1536, whose whole tiles do not fit the register budget (768^3: fused pass 29.5 ->
        // 23.7 ms, apply 56.3 -> 50.4 ms); at L = 1024 it ties with 3 (5.19-5.25 against 5.20-5.25 ms; it moves 24.0 GB instead
        // of 25.8: paired rows meet in L2) and 3 stays (profiles/r02_experiment_ticketed_half_tiles.log)
        // (the 1280-point line, 20 elements per thread, likewise: 640^3 fused pass 18.5 -> 16.5 ms, apply 35.6 -> 33.6 ms)
        // 6 = 3 with the tiles handed out by the same tickets (row pairs per XCD: both reads of a symbol row meet in one L2):
        // 512^3 apply 12.95 -> 12.86 ms over three A/B rounds of bench.py, neutral at 256^3; auto from L = 1024 on
        const int zp = tn.z_persist >= 0 ? tn.z_persist : ((L == 1536 || L == 1280 || L == 2048) ? 5 : (L >= 1024 ? 6 : 3));   // (2048: 1024^3 fused pass 58.8 -> 47.0 ms)
        const bool eight_lines = t.lines == XB;
        // (worth it only when a workgroup walks over several tiles: below ~4 tiles per resident workgroup -- grids up to 64^3 --
        // the one-tile kernels finish sooner, 35 against 37.5 us per apply at 48^3)
        const bool enough_tiles = tn.z_persist > 0 || ntiles >= (int64_t)4096;
        // 5: half tiles (4-line workgroups, swizzled unpadded exchange buffer + twiddle table), two workgroups per CU at L = 1024;
        // below 1024 points (whole tiles only) and on grids without a multiple of 16 tiles in row pairs a request for 5 runs as 4
        const bool half5 = zp == 5 && tiled && have_twl && L >= 1024 && ntiles % 16 == 0 && (g.nouter % 2 == 0 || !g.ytab);
        if (zp > 0 && g.zm && g.dLine == 8 && nrhs == 1 && (eight_lines || half5) && (!half_form || half5) && enough_tiles) {
            if (half5) {
                f.family = PassFamily::ZFUSED_PERSIST_HALF; f.lines = XB / 2; f.wpe = t.persist_half_wpe;
                f.twl = f.late_sym = f.tickets = true;
                f.xl = (tn.xlane != 0 && t.xl_persist_half) ? 1 : 0;
                return f;
            }
            f.family = PassFamily::ZFUSED_PERSIST; f.lines = XB;
            const bool split = zp == 2 || zp == 4 || t.xb_full_lds > LDS_BYTES;
            int xlreq = 0;
            // 6: whole tiles (as 3) handed out by tickets in row pairs per XCD; without a multiple of 16 tiles in row pairs it runs as 3
            if (zp == 6 && !split && ntiles % 16 == 0 && g.nouter % 2 == 0) { f.late_sym = f.tickets = true; xlreq = tn.xlane < 0 ? 5 : tn.xlane; }
            else if ((zp == 3 || zp == 6) && !split) { f.late_sym = true; xlreq = tn.xlane < 0 ? 1 : tn.xlane; }
            else if (zp >= 3) { f.split = f.late_sym = true; }
            else f.split = split;
            f.twl = tn.tw_lds && have_twl && t.persist_lds[f.split] + (size_t)t.twlen * sizeof(cplx) <= LDS_BYTES;
            // lane exchanges between stages of equal radix (whole-complex whole tiles, symbol after the first stage: the 512^3 and 256^3 forms)
            f.xl = persist_xl(xlreq, t.xl_persist && !f.split && f.late_sym, f.twl, f.tickets);
            return f;
        }
    }
    if (nrhs > 1 && half_form) {
        FusedPass one = a; one.nrhs = 1;
        f = zfused_form(tn, one);
        f.per_member = true;
        return f;
    }
    if (zh > 0) {
        f.family = PassFamily::ZFUSED_HALF; f.lines = XB / 2;
        f.split = zh == 2 || zh == 3; f.prefetch = zh == 1 || zh == 2;
        f.wpe = L == 1024 ? (zh == 3 ? 3 : 2) : 1;
        f.xl = (!f.split && t.xl_half) ? 1 : 0;
        return f;
    }
    if (half2048) {
        // LSFC_Z_QUARTER=1 (experiment, off): quarter tiles, two 256-thread workgroups per CU (74 KB of LDS each).  Measured on
        // the 2D tiled pass at n = 1024 (256 tiles): 35.4 against 34.2 us -- workgroups that start together run their phases
        // together, so two per CU overlap nothing in a one-tile kernel; the ticketed persistent form (2 half tiles per
        // workgroup) takes 54.8 us there (profiles/r02_2d_half_symbol.jsonl)
        const bool quarter = g.zm && env_flag_z_quarter();
        f.family = PassFamily::ZFUSED_HALF; f.lines = quarter ? 2 : XB / 2; f.wpe = 2;
        f.xl = (quarter ? t.xl_quarter : t.xl_half) ? 1 : 0;
        return f;
    }
    // auto (-1): measured on MI355X -- at L >= 1024 (16 elements/thread, 2 waves/SIMD either way) whole-complex
    // exchanges + symbol prefetch win (7.4 -> 6.7 ms at 512^3); below, split exchanges without prefetch (more waves)
    // mixed-radix lines (profiles/r01_experiment_mixed_radix_knobs.log): the symbol prefetch pays from L = 320 on
    // (z pass -15..-30 %), whole-complex exchanges on the factor-3 lines from L = 384; the 1536-point line (24
    // elements per thread in 512-thread workgroups) has no registers left for the prefetch
#if LSFC_FAMILY == 2
    // (the 2048-point line reaches this point only in the 2D layout, 4 lines per workgroup: no prefetch there,
    // fused pass 54 -> 46 us at 2D n = 1024)
    const bool e16 = L == 1024, full = L >= 1024;
#elif LSFC_FAMILY == 3
    const bool e16 = L >= 384 && L < 1536, full = L >= 384;
#else
    const bool e16 = L >= 320, full = false;
#endif
    f.family = PassFamily::ZFUSED; f.lines = t.lines;
    f.split = tn.split_z >= 0 ? tn.split_z != 0 : !full;
    // whole-complex exchange buffers of the longest lines exceed the 160 KiB of LDS: those run split
    // (sized by the workgroup zfused_t launches: Tune<C>::LINES lines -- the y passes alone use YLINES)
    if (t.tile_lds[0] > LDS_BYTES) f.split = true;
    // batch: one symbol load per tile for all right-hand sides, always up front (no PREFETCH flavour)
    f.batch = nrhs > 1;
    f.prefetch = !f.batch && (tn.sym_prefetch >= 0 ? tn.sym_prefetch != 0 : e16);
    f.twl = tn.tw_lds && have_twl && t.tile_lds[f.split] + (size_t)t.twlen * sizeof(cplx) <= LDS_BYTES;   // the table must fit beside the exchange buffer
    f.xl = (!f.split && t.xl_tile) ? 1 : 0;
    return f;
}

// The half-tile one-tile kernels that exist, (line, SPLIT, PREFETCH, WPE, LINES): each with the full and the z-even symbol, the
// quarter tiles of the 2048-point line with the z-even symbol only
template <class C_, bool SPLIT_, bool PREFETCH_, int WPE_, int LINES_ = 4> struct HalfTile {
    using C = C_;
    static constexpr bool SPLIT = SPLIT_, PREFETCH = PREFETCH_;
    static constexpr int WPE = WPE_, LINES = LINES_;
};
template <class... H> struct HalfTiles {};
#if LSFC_FAMILY == 2
using FamilyHalfTiles = HalfTiles<HalfTile<Cfg1024, true, true, 2>, HalfTile<Cfg1024, true, false, 3>, HalfTile<Cfg1024, false, true, 2>, HalfTile<Cfg1024, false, false, 2>,
                                  HalfTile<Cfg2048, false, false, 2>, HalfTile<Cfg2048, false, false, 2, 2>>;
#elif LSFC_FAMILY == 3
using FamilyHalfTiles = HalfTiles<HalfTile<Cfg1536, true, true, 1>, HalfTile<Cfg1536, true, false, 1>, HalfTile<Cfg1536, false, true, 1>, HalfTile<Cfg1536, false, false, 1>>;
#else
using FamilyHalfTiles = HalfTiles<>;
#endif
template <class H> static bool zfused_half_try(const PassForm& f, const FusedPass& a, hipStream_t st) {
    if (f.L != H::C::L || f.split != H::SPLIT || f.prefetch != H::PREFETCH || f.wpe != H::WPE || f.lines != H::LINES) return false;
    LSFC_REQUIRE(H::LINES == 4 || f.ze, "internal: quarter-tile fused pass without the z-even symbol");
    dispatch_flags({f.ze, f.full}, [&](auto ZE, auto FULL) {
        if constexpr (H::LINES == 4 || ZE) zfused_half_t<typename H::C, H::SPLIT, H::PREFETCH, H::WPE, ZE, H::LINES, FULL>(a, st);
    });
    return true;
}
template <class... H> static void zfused_half(HalfTiles<H...>, const PassForm& f, const FusedPass& a, hipStream_t st) {
    if (!(zfused_half_try<H>(f, a, st) || ...))
        fail(LSFC_EINVAL, "internal: no half-tile fused kernel of flavour %d at %d points", (f.split ? 100 : 0) + (f.prefetch ? 10 : 0) + f.wpe, f.L);
}

static void zfused(const PrunedTuning& tn, const FusedPass& a, hipStream_t st) {
    const PassForm f = zfused_form(tn, a);
    if (f.per_member) {
        for (int r = 0; r < a.nrhs; ++r) {
            FusedPass one = a; one.data = a.data + (int64_t)r * a.dBatch; one.nrhs = 1; one.dBatch = 0;
            zfused(tn, one, st);
        }
        return;
    }
    switch (f.family) {
    case PassFamily::ZFUSED_PERSIST_HALF:
        dispatch_line(a.L, [&](auto c) { zfused_persist_half_t<decltype(c)>(f, a, st); });
        break;
    case PassFamily::ZFUSED_PERSIST:
        LSFC_REQUIRE(f.wpe == 1 && f.lines == XB, "internal: persistent whole tiles run %d lines, %d workgroups per CU", f.lines, f.wpe);
        dispatch_line(a.L, [&](auto c) { dispatch_flags({f.split, f.late_sym, f.tickets}, [&](auto SPLIT, auto LATE_SYM, auto TICKETS) {
            // (tickets: whole-complex exchanges with the symbol after the first stage only)
            if constexpr (!TICKETS || (!SPLIT && LATE_SYM)) zfused_persist_t<decltype(c), SPLIT, LATE_SYM, TICKETS>(f, a, st);
            else fail(LSFC_EINVAL, "internal: no ticketed persistent fused kernel with SPLIT=%d LATE_SYM=%d", (int)SPLIT, (int)LATE_SYM);
        }); });
        break;
    case PassFamily::ZFUSED_HALF:
        zfused_half(FamilyHalfTiles{}, f, a, st);
        break;
    case PassFamily::ZFUSED:
        LSFC_REQUIRE(f.wpe == 1, "internal: one-tile fused kernels are bounded for one workgroup per CU, not %d", f.wpe);
        dispatch_line(a.L, [&](auto c) { dispatch_flags({f.split, f.prefetch, f.ze}, [&](auto SPLIT, auto PREFETCH, auto ZE) {
            zfused_t<decltype(c), SPLIT, PREFETCH, 1, ZE>(f, a, st);
        }); });
        break;
    default:
        fail(LSFC_EINVAL, "internal: %s is not a form of the fused pass", pass_family_name(f.family));
    }
    LSFC_HIP(hipGetLastError());
}

// the one symbol this compilation exports (pruned.hpp); host only -- the device pass would emit the constant into the code object too
#ifndef __HIP_DEVICE_COMPILE__
extern const PrunedFamily FAM(pruned_family) = {.xfwd = xfwd, .xinv = xinv, .yfwd = yfwd, .yinv = yinv, .zfused = zfused,
                                                .xform = xform, .yform = yform, .zfused_form = zfused_form,
                                                .perm = perm, .twfull_len = twfull_len, .twfull = twfull, .warmup = warmup};
#endif

} // namespace lsfc
