// The sweeps of the block-tridiagonal preconditioner: x <- Msp^{-1} w (and Msp^{-T} w) from the inverses S_k^{-1} that
// blocktri_factor.hip stored (the elimination: blocktri.hpp).  2 K - 1 steps per apply, inside every Krylov iteration.
//
// The sweeps widen every stored entry to fp64 on load and sum in fp64 in the order of the fp64 object.  There is one sweep
// kernel per shape, a template over the stored type T (k_bt_walk<T>, k_bt_step<FWD, T>, k_btb_product<R, T>), and the
// enqueue functions pick T once (with_storage).  The storages differ in the load alone: a lane's 16 B load is one row of
// complex double, or rows i and i + 1 of float pairs (BT_LANE_ROWS<T>; bt_accum / bt_accum2 in the step, the column loop in
// the product), so a workgroup covers twice the rows at float storage.  Staging, chunk loop, accumulators, LDS fold and
// store are shared.
//
// Apply: one kernel per step of the two sweeps; a workgroup forms the stencil product (L_k z_{k-1} or U_k x_{k+1}) in
// LDS and multiplies 16 lanes of rows of S_k^{-1} with it (16 B loads: 16 rows of complex double, 32 of float pairs; 32
// column slots folded through LDS in a fixed order, one row of a lane after the other).
// Planes of at most 96 rows are walked inside one launch by a single workgroup, one row per lane at either storage.
//
// Apply to a GROUP of up to 8 right-hand sides (blocktri_enqueue_batch): three launches per step.  A small kernel forms the
// stencil product once for all members (b x R), the product kernel reads S_k^{-1} once and applies every loaded entry to
// all R members (tiles of 64 lanes of rows -- 64 rows of complex double, 128 of float pairs -- x a range of columns, so
// that one step fills the device), a third kernel folds the column ranges in a fixed order.  What is summed for one
// member, and in which order, is fixed by b alone.
#include "blocktri_object.hpp"
#include <algorithm>

namespace lsfc {

static constexpr int AP_ROWS = 16;        // apply: rows of S_k^{-1} per workgroup ...
static constexpr int AP_SLOTS = 32;       // ... times column slots = 512 threads
static constexpr int AP_CHUNK = 2048;     // apply: entries of the stencil product staged in LDS at a time
static constexpr int WALK_B = 96;         // planes of at most this many rows: both sweeps inside one launch

// ---- the apply -----------------------------------------------------------------------------------------------------

// a stored entry of S_k^{-1} as fp64: the float form is widened (exact), all arithmetic after it is fp64
typedef float f4u __attribute__((ext_vector_type(4), aligned(8)));           // two consecutive float pairs of one column
__device__ __forceinline__ cplx bt_ld(const cplx* p) { return *p; }
__device__ __forceinline__ cplx bt_ld(const cplx32* p) { const cplx32 v = *p; return make_double2((double)v.x, (double)v.y); }

// entries [jc, jc + n) of the right-hand side of step k into LDS: w_k - L_k z_{k-1} (forward) or U_k x_{k+1} (backward)
template <bool FWD>
__device__ __forceinline__ void bt_stage(const BtApply& a, int k, int64_t jc, int n, const cplx* __restrict__ w, const cplx* x, cplx* t) {
    for (int jj = threadIdx.x; jj < n; jj += AP_ROWS * AP_SLOTS) {
        const int64_t g = (int64_t)k * a.b + jc + jj;
        cplx s;
        if (FWD) {
            s = w[g];
            if (k > 0) { cplx u = make_double2(0.0, 0.0); for (int64_t q = a.rowptr[g]; q < a.rlo[g]; ++q) cfma(u, a.val[q], x[a.col[q]]); s.x -= u.x; s.y -= u.y; }
        } else {
            s = make_double2(0.0, 0.0);
            for (int64_t q = a.rhi[g]; q < a.rowptr[g + 1]; ++q) cfma(s, a.val[q], x[a.col[q]]);
        }
        t[jj] = s;
    }
}

// this thread's share of (S_k^{-1} t)[i]: columns jc + slot, jc + slot + 32, ...
template <typename T>
__device__ __forceinline__ void bt_accum(const T* __restrict__ Sk, int64_t b, int64_t i, int64_t jc, int n, int slot, const cplx* t, cplx& acc) {
    if (i >= b) return;
    const T* p = Sk + i + (jc + slot) * b;
#pragma unroll 4
    for (int jj = slot; jj < n; jj += AP_SLOTS, p += (int64_t)AP_SLOTS * b) cfma(acc, bt_ld(p), t[jj]);
}

// float storage: rows i and i + 1 of the same columns from one 16 B load (i + 1 < b), each row summed as bt_accum sums it
__device__ __forceinline__ void bt_accum2(const cplx32* __restrict__ Sk, int64_t b, int64_t i, int64_t jc, int n, int slot, const cplx* t,
                                          cplx& acc0, cplx& acc1) {
    const cplx32* p = Sk + i + (jc + slot) * b;
#pragma unroll 4
    for (int jj = slot; jj < n; jj += AP_SLOTS, p += (int64_t)AP_SLOTS * b) {
        const f4u v = *(const f4u*)p;
        const cplx tj = t[jj];
        cfma(acc0, make_double2((double)v.x, (double)v.y), tj);
        cfma(acc1, make_double2((double)v.z, (double)v.w), tj);
    }
}

// fold the 32 column slots of every row in slot order; the sum is valid on the threads of slot 0
__device__ __forceinline__ cplx bt_fold(cplx acc, cplx* red) {
    red[threadIdx.x] = acc;
    __syncthreads();
    cplx s = make_double2(0.0, 0.0);
    if (threadIdx.x < AP_ROWS) for (int q = 0; q < AP_SLOTS; ++q) { const cplx v = red[q * AP_ROWS + threadIdx.x]; s.x += v.x; s.y += v.y; }
    __syncthreads();
    return s;
}

// rows of S_k^{-1} that a lane of the step and product kernels takes with one 16 B load: one row of complex double, or
// rows i and i + 1 of float pairs.  The load is all that the two storages do differently.
template <typename T> constexpr int BT_LANE_ROWS = (int)(sizeof(cplx) / sizeof(T));

// one step of a sweep over many workgroups, 16 lanes of rows each (a quarter wave reads 256 B of a column): forward writes
// z_k, backward updates it in place to x_k (a workgroup writes rows of block k only and reads block k -+ 1 only)
template <bool FWD, typename T>
__global__ __launch_bounds__(AP_ROWS * AP_SLOTS) void k_bt_step(BtApply a, const T* __restrict__ S, int k, const cplx* __restrict__ w, cplx* x) {
    constexpr int LR = BT_LANE_ROWS<T>;
    __shared__ cplx t[AP_CHUNK], red[AP_ROWS * AP_SLOTS];
    const int r = threadIdx.x & (AP_ROWS - 1), slot = threadIdx.x / AP_ROWS;
    const int64_t i = ((int64_t)blockIdx.x * AP_ROWS + r) * LR;
    const T* Sk = S + (int64_t)k * a.b * a.b;
    cplx acc[LR];
#pragma unroll
    for (int h = 0; h < LR; ++h) acc[h] = make_double2(0.0, 0.0);
    for (int64_t jc = 0; jc < a.b; jc += AP_CHUNK) {
        const int n = (int)(a.b - jc < AP_CHUNK ? a.b - jc : AP_CHUNK);
        bt_stage<FWD>(a, k, jc, n, w, x, t);
        __syncthreads();
        if constexpr (LR == 2) {
            if (i + 1 < a.b) bt_accum2(Sk, a.b, i, jc, n, slot, t, acc[0], acc[1]);
            else bt_accum(Sk, a.b, i, jc, n, slot, t, acc[0]);              // the last row of an odd plane, or none
        } else bt_accum(Sk, a.b, i, jc, n, slot, t, acc[0]);
        __syncthreads();
    }
#pragma unroll
    for (int h = 0; h < LR; ++h) {
        const cplx s = bt_fold(acc[h], red);
        if (slot == 0 && i + h < a.b) {
            cplx& o = x[(int64_t)k * a.b + i + h];
            if (FWD) o = s; else { o.x -= s.x; o.y -= s.y; }
        }
    }
}

// small planes (b <= WALK_B): both sweeps by ONE workgroup, a barrier between steps.  One shape for both storages: a
// single workgroup waits on the chain of steps, not on bytes, so the float form keeps one row per thread (8 B loads).
template <typename T>
__global__ __launch_bounds__(AP_ROWS * AP_SLOTS) void k_bt_walk(BtApply a, const T* __restrict__ S, const cplx* __restrict__ w, cplx* x) {
    __shared__ cplx t[WALK_B], red[AP_ROWS * AP_SLOTS];
    const int r = threadIdx.x & (AP_ROWS - 1), slot = threadIdx.x / AP_ROWS;
    const int b = (int)a.b;
    for (int step = 0; step < 2 * a.K - 1; ++step) {
        const bool fwd = step < a.K;
        const int k = fwd ? step : 2 * a.K - 2 - step;
        if (fwd) bt_stage<true>(a, k, 0, b, w, x, t); else bt_stage<false>(a, k, 0, b, w, x, t);
        __syncthreads();
        const T* Sk = S + (int64_t)k * b * b;
        for (int i0 = 0; i0 < b; i0 += AP_ROWS) {
            cplx acc = make_double2(0.0, 0.0);
            bt_accum(Sk, b, i0 + r, 0, b, slot, t, acc);
            const cplx s = bt_fold(acc, red);
            if (slot == 0 && i0 + r < b) {
                cplx& o = x[(int64_t)k * b + i0 + r];
                if (fwd) o = s; else { o.x -= s.x; o.y -= s.y; }
            }
        }
        __syncthreads();                          // this step's rows are visible to the next step (same workgroup)
    }
}

// ---- the transposed apply: x <- Msp^{-T} w -----------------------------------------------------------------------------
//
//     forward   z_k = S_k^{-T} (w_k - U_{k-1}^T z_{k-1})        backward   x_k = z_k - S_k^{-T} (L_{k+1}^T x_{k+1})
//
// on the same stored S_k^{-1}.  BtApply then holds the CSR of Msp^T (its "lower" part is U_{k-1}^T, its "upper" part
// L_{k+1}^T), so bt_stage and k_btb_stage are the ones above.  The dense product y[j] = sum_i S_k^{-1}[i + j b] t[i] sums
// along the contiguous axis: a wave walks down columns, 16 B per lane and column (one row of complex double, or rows
// i, i + 1 of float pairs, both for the same output), several columns in flight so that one LDS read of t feeds them all,
// and the per-lane partial sums are folded across the wave at the end.

// Sums over the 64 lanes of a wave of P doubles per lane (P a power of two, at most 64), by the butterfly 1, 2, 4, ..., 32 in
// which the partners split the values between them while there are several: P - 1 + (6 - log2 P) cross-lane moves instead
// of 6 P, and the steps with the most values to move are the ones inside a quad, which are DPP moves on the VALU and not
// trips through the LDS crossbar.  Every sum is the one the plain butterfly of that order gives, whatever P.  Afterwards
// v[0] of lane L is the sum of value bt_scatter_index<P>(L) (lanes that agree in their low log2 P bits hold the same one).
template <int O>
__device__ __forceinline__ double bt_xor_lane(double x) {                         // x of lane ^ O
    if constexpr (O == 1 || O == 2) {
        constexpr int quad_perm = O == 1 ? 0xB1 : 0x4E;                           // [1, 0, 3, 2] and [2, 3, 0, 1]
        const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), quad_perm, 0xF, 0xF, false);
        const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), quad_perm, 0xF, 0xF, false);
        return __hiloint2double(hi, lo);
    } else return __shfl_xor(x, O, 64);
}
template <int H, int O, int P>
__device__ __forceinline__ void bt_wave_sums_step(double (&v)[P], int lane) {      // the step with partner lane ^ O, H values kept
    if constexpr (O <= 32) {
        if constexpr (H >= 1) {
            const bool up = (lane & O) != 0;
#pragma unroll
            for (int m = 0; m < H; ++m) {
                const double send = up ? v[m] : v[m + H], keep = up ? v[m + H] : v[m];
                v[m] = keep + bt_xor_lane<O>(send);
            }
        } else v[0] += bt_xor_lane<O>(v[0]);
        bt_wave_sums_step<H / 2, O * 2>(v, lane);
    }
}
template <int P>
__device__ __forceinline__ void bt_wave_sums(double (&v)[P]) {
    static_assert(P >= 1 && P <= 64 && (P & (P - 1)) == 0, "a power of two up to the wave size");
    bt_wave_sums_step<P / 2, 1>(v, threadIdx.x & 63);
}
template <int P>
__device__ __forceinline__ int bt_scatter_index(int lane) {
    int idx = 0;
#pragma unroll
    for (int h = P / 2, o = 1; h >= 1; h >>= 1, o <<= 1) idx += (lane & o) ? h : 0;
    return idx;
}
template <int P> constexpr int BT_HOLDER_MASK = 63 & ~(P - 1);                    // lanes with these bits clear (lane < P) write the sums
constexpr int bt_pow2(int n) { int p = 1; while (p < n) p <<= 1; return p; }

static constexpr int ST_WAVES = AP_ROWS * AP_SLOTS / 64;   // the waves of a workgroup share its columns and split the rows
static constexpr int ST_COLS = 16;        // columns of S_k^{-1} per workgroup, all in flight on every wave
static constexpr int WT_COLS = 4;         // walk kernel: columns in flight per wave

// this wave's share of sum_i S_k^{-1}[ic + i, j0 + c] t[i], i < n, for the ncol columns of the workgroup: chunks of
// 64 lane loads (64 or 128 rows), chunk q on wave q mod 8, a lane's chunks in ascending order
// FULL: all 16 columns exist -- the 16 loads of a lane are issued together, ahead of the first multiply-add.  The last
// workgroup of a plane whose size is no multiple of 16 takes its columns one by one.
template <bool FULL, typename T>
__device__ __forceinline__ void bt_accum_t(const T* __restrict__ Sk, int64_t b, int64_t j0, int ncol, int64_t ic, int n, const cplx* t,
                                           cplx (&acc)[ST_COLS]) {
    constexpr int LR = BT_LANE_ROWS<T>;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int ii = (wave * 64 + lane) * LR; ii < n; ii += ST_WAVES * 64 * LR) {
        const T* p = Sk + ic + ii + j0 * b;
        const cplx t0 = t[ii];
        if constexpr (LR == 2) {
            if (ii + 1 < n) {                                              // (n is even unless the plane ends here)
                const cplx t1 = t[ii + 1];
                if constexpr (FULL) {
                    f4u v[ST_COLS];
#pragma unroll
                    for (int c = 0; c < ST_COLS; ++c) v[c] = *(const f4u*)(p + (int64_t)c * b);
#pragma unroll
                    for (int c = 0; c < ST_COLS; ++c) {
                        cfma(acc[c], make_double2((double)v[c].x, (double)v[c].y), t0);
                        cfma(acc[c], make_double2((double)v[c].z, (double)v[c].w), t1);
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < ST_COLS; ++c) if (c < ncol) {
                        const f4u v = *(const f4u*)(p + (int64_t)c * b);
                        cfma(acc[c], make_double2((double)v.x, (double)v.y), t0);
                        cfma(acc[c], make_double2((double)v.z, (double)v.w), t1);
                    }
                }
                continue;
            }
        }
        if constexpr (FULL) {
            cplx v[ST_COLS];
#pragma unroll
            for (int c = 0; c < ST_COLS; ++c) v[c] = bt_ld(p + (int64_t)c * b);
#pragma unroll
            for (int c = 0; c < ST_COLS; ++c) cfma(acc[c], v[c], t0);
        } else {
#pragma unroll
            for (int c = 0; c < ST_COLS; ++c) if (c < ncol) cfma(acc[c], bt_ld(p + (int64_t)c * b), t0);
        }
    }
}

// one step of a transposed sweep over many workgroups: 16 columns each, the 8 waves take the row chunks in turn.  The lanes
// of a wave are folded by bt_wave_sums, the waves through LDS in wave order.
template <bool FWD, typename T>
__global__ __launch_bounds__(AP_ROWS * AP_SLOTS) void k_bt_step_t(BtApply a, const T* __restrict__ S, int k, const cplx* __restrict__ w, cplx* x) {
    __shared__ cplx t[AP_CHUNK];
    __shared__ double red[ST_WAVES][2 * ST_COLS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t j0 = (int64_t)blockIdx.x * ST_COLS;
    const int ncol = (int)(a.b - j0 < ST_COLS ? a.b - j0 : ST_COLS);
    const T* Sk = S + (int64_t)k * a.b * a.b;
    cplx acc[ST_COLS];
#pragma unroll
    for (int c = 0; c < ST_COLS; ++c) acc[c] = make_double2(0.0, 0.0);
    for (int64_t ic = 0; ic < a.b; ic += AP_CHUNK) {
        const int n = (int)(a.b - ic < AP_CHUNK ? a.b - ic : AP_CHUNK);
        bt_stage<FWD>(a, k, ic, n, w, x, t);
        __syncthreads();
        if (ncol == ST_COLS) bt_accum_t<true>(Sk, a.b, j0, ncol, ic, n, t, acc); else bt_accum_t<false>(Sk, a.b, j0, ncol, ic, n, t, acc);
        __syncthreads();
    }
    double v[2 * ST_COLS];
#pragma unroll
    for (int c = 0; c < ST_COLS; ++c) { v[2 * c] = acc[c].x; v[2 * c + 1] = acc[c].y; }
    bt_wave_sums(v);
    if ((lane & BT_HOLDER_MASK<2 * ST_COLS>) == 0) red[wave][bt_scatter_index<2 * ST_COLS>(lane)] = v[0];
    __syncthreads();
    if ((int)threadIdx.x < ncol) {
        cplx s = make_double2(0.0, 0.0);
        for (int q = 0; q < ST_WAVES; ++q) { s.x += red[q][2 * threadIdx.x]; s.y += red[q][2 * threadIdx.x + 1]; }
        cplx& o = x[(int64_t)k * a.b + j0 + threadIdx.x];
        if (FWD) o = s; else { o.x -= s.x; o.y -= s.y; }
    }
}

// small planes (b <= WALK_B): both transposed sweeps by ONE workgroup.  Wave q takes the columns 4 q .. 4 q + 3, then
// 32 columns on; one row per lane and load at either storage, as in k_bt_walk.
template <typename T>
__global__ __launch_bounds__(AP_ROWS * AP_SLOTS) void k_bt_walk_t(BtApply a, const T* __restrict__ S, const cplx* __restrict__ w, cplx* x) {
    __shared__ cplx t[WALK_B];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = (int)a.b;
    for (int step = 0; step < 2 * a.K - 1; ++step) {
        const bool fwd = step < a.K;
        const int k = fwd ? step : 2 * a.K - 2 - step;
        if (fwd) bt_stage<true>(a, k, 0, b, w, x, t); else bt_stage<false>(a, k, 0, b, w, x, t);
        __syncthreads();
        const T* Sk = S + (int64_t)k * b * b;
        for (int j0 = wave * WT_COLS; j0 < b; j0 += ST_WAVES * WT_COLS) {          // (uniform over the wave)
            double v[2 * WT_COLS];
#pragma unroll
            for (int c = 0; c < 2 * WT_COLS; ++c) v[c] = 0.0;
            for (int i = lane; i < b; i += 64) {
                const cplx ti = t[i];
#pragma unroll
                for (int c = 0; c < WT_COLS; ++c) if (j0 + c < b) {
                    cplx s = make_double2(v[2 * c], v[2 * c + 1]);
                    cfma(s, bt_ld(Sk + i + (int64_t)(j0 + c) * b), ti);
                    v[2 * c] = s.x; v[2 * c + 1] = s.y;
                }
            }
            bt_wave_sums(v);
            const int idx = bt_scatter_index<2 * WT_COLS>(lane), j = j0 + idx / 2;
            if ((lane & BT_HOLDER_MASK<2 * WT_COLS>) == 0 && j < b) {
                double* o = (double*)&x[(int64_t)k * b + j] + (idx & 1);
                if (fwd) *o = v[0]; else *o -= v[0];
            }
        }
        __syncthreads();                          // this step's rows are visible to the next step (same workgroup)
    }
}

// ---- the apply for a group of right-hand sides -------------------------------------------------------------------------
//
// Vectors of a group are member-major (member r at offset r N); the stencil product t is b x R with the R values of a row
// next to each other.  A member's result must not depend on its companions (a lock-step GMRES drops converged members):
// the tiling below comes from b alone, every member has its own accumulators, and the complex multiply-adds are spelled
// as fused multiply-adds, so no instantiation contracts them differently from another.

static constexpr int BB_ROWS = 64;        // rows of S_k^{-1} per workgroup: one wave along a column, 1 KiB per load ...
static constexpr int BB_SLOTS = 4;        // ... times column slots (waves) = 256 threads
static constexpr int BB_COLS_MAX = 128;   // columns of S_k^{-1} per workgroup at most

// columns per workgroup (from b alone): b / 64 row tiles times b / cols column ranges keep 256 CUs busy from b ~ 600 on
static int bb_cols(int64_t b) { return b < 1024 ? 32 : (b < 2048 ? 64 : BB_COLS_MAX); }

__device__ __forceinline__ void cfma_x(cplx& s, cplx a, cplx b) {
    s.x = fma(a.x, b.x, s.x); s.x = fma(-a.y, b.y, s.x);
    s.y = fma(a.x, b.y, s.y); s.y = fma(a.y, b.x, s.y);
}

// t[j, r] = (w_r)_k[j] - (L_k (z_r)_{k-1})[j] (forward) or (U_k (x_r)_{k+1})[j] (backward): a thread per row and member
template <bool FWD>
__global__ __launch_bounds__(256) void k_btb_stage(BtApply a, int k, int R, int64_t N, const cplx* __restrict__ w, const cplx* __restrict__ x,
                                                   cplx* __restrict__ t) {
    const int64_t idx = blockIdx.x * (int64_t)256 + threadIdx.x;
    if (idx >= a.b * R) return;
    const int r = (int)(idx % R);
    const int64_t g = (int64_t)k * a.b + idx / R;
    const cplx* xr = x + (int64_t)r * N;
    cplx s;
    if (FWD) {
        s = w[(int64_t)r * N + g];
        if (k > 0) { cplx u = make_double2(0.0, 0.0); for (int64_t q = a.rowptr[g]; q < a.rlo[g]; ++q) cfma_x(u, a.val[q], xr[a.col[q]]); s.x -= u.x; s.y -= u.y; }
    } else {
        s = make_double2(0.0, 0.0);
        for (int64_t q = a.rhi[g]; q < a.rowptr[g + 1]; ++q) cfma_x(s, a.val[q], xr[a.col[q]]);
    }
    t[idx] = s;
}

// part[c, r, i] = sum over the columns j of range c of S_k^{-1}[i, j] t[j, r].  Workgroup (row tile, column range): the
// range's rows of t go to LDS, wave `slot` takes the columns slot, slot + 4, ... of the range, lane = row: a wave reads
// 64 lanes of consecutive rows of one column (16 B per lane, 1 KiB per wave: 64 rows of complex double, or 128 rows of
// float pairs with rows i, i + 1 on a lane) and applies every entry to the R members (R accumulators per row, the R values
// of t read from LDS at one address for the whole wave).  The four slots are folded through LDS in slot order, one row
// of a lane after the other.  A row's sum runs over the same columns, slots and ranges in the same order at either
// storage, and the tiling is a function of b alone, so a member's bits do not depend on its companions.
template <int R, typename T>
__global__ __launch_bounds__(BB_ROWS * BB_SLOTS) void k_btb_product(const T* __restrict__ Sk, int64_t b, int cols, const cplx* __restrict__ t,
                                                                    cplx* __restrict__ part) {
    constexpr int LR = BT_LANE_ROWS<T>;
    __shared__ cplx ts[BB_COLS_MAX * R], red[(BB_SLOTS - 1) * R * BB_ROWS];
    const int lane = threadIdx.x & (BB_ROWS - 1), slot = threadIdx.x / BB_ROWS;
    const int64_t i = ((int64_t)blockIdx.x * BB_ROWS + lane) * LR, jc = (int64_t)blockIdx.y * cols;
    const int n = (int)(b - jc < cols ? b - jc : cols);
    for (int e = threadIdx.x; e < n * R; e += BB_ROWS * BB_SLOTS) ts[e] = t[jc * R + e];
    __syncthreads();
    cplx acc[LR][R];
#pragma unroll
    for (int h = 0; h < LR; ++h)
#pragma unroll
        for (int r = 0; r < R; ++r) acc[h][r] = make_double2(0.0, 0.0);
    bool paired = false;
    if constexpr (LR == 2) {
        if (i + 1 < b) {
            paired = true;
            const T* p = Sk + i + (jc + slot) * b;
#pragma unroll 4
            for (int jj = slot; jj < n; jj += BB_SLOTS, p += (int64_t)BB_SLOTS * b) {
                const f4u v = *(const f4u*)p;
                const cplx s0 = make_double2((double)v.x, (double)v.y), s1 = make_double2((double)v.z, (double)v.w);
#pragma unroll
                for (int r = 0; r < R; ++r) { const cplx tj = ts[jj * R + r]; cfma_x(acc[0][r], s0, tj); cfma_x(acc[1][r], s1, tj); }
            }
        }
    }
    if (!paired && i < b) {                                                   // one row: complex double, or the last row of an odd plane
        const T* p = Sk + i + (jc + slot) * b;
#pragma unroll 4
        for (int jj = slot; jj < n; jj += BB_SLOTS, p += (int64_t)BB_SLOTS * b) {
            const cplx s = bt_ld(p);
#pragma unroll
            for (int r = 0; r < R; ++r) cfma_x(acc[0][r], s, ts[jj * R + r]);
        }
    }
#pragma unroll
    for (int h = 0; h < LR; ++h) {
        if (slot > 0) {
#pragma unroll
            for (int r = 0; r < R; ++r) red[((slot - 1) * R + r) * BB_ROWS + lane] = acc[h][r];
        }
        __syncthreads();
        if (slot == 0 && i + h < b) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                cplx s = acc[h][r];
                for (int q = 0; q < BB_SLOTS - 1; ++q) { const cplx v = red[(q * R + r) * BB_ROWS + lane]; s.x += v.x; s.y += v.y; }
                part[((int64_t)blockIdx.y * R + r) * b + i + h] = s;
            }
        }
        if (h + 1 < LR) __syncthreads();                                      // red is free for the lane's next row
    }
}

// The transposed group product: part[c, r, j] = sum over the rows i of range c of S_k^{-1}[i, j] t[i, r].  Workgroup
// (column tile, row range): the range's rows of t go to LDS member by member (a wave reads the 64 or 128 values of one
// member at consecutive addresses), each of the four waves takes `wcols` columns of the tile, two at a time: a lane loads
// its 16 B of each column for the whole range first, then applies every entry to the R members.  At float storage a range
// is half as many lane loads, so a wave takes four columns at a time there: 8 loads of 16 B per lane in flight and 2 R or
// 4 R accumulators at either storage.  The lanes are folded by
// bt_wave_sums and the sums go straight to `part`: no wave shares a column with another.  Ranges are folded by k_btb_fold.
// Tile and range come from b alone and the multiply-adds are spelled out, so a member's bits do not depend on its companions.
static constexpr int BT_WAVES = 4;        // waves per workgroup, each with its own columns
static constexpr int BT_CJ = 2;           // columns in flight per wave at complex double (2 R accumulators), twice as many of float pairs
static constexpr int BT_RANGE_MAX = 256;  // rows of S_k^{-1} per workgroup at most (R = 8: 32 KiB of t in LDS)

// tile and range from b alone: b / 32 x b / 128 workgroups below 2048 rows (256 of them at b = 1024), b / 64 x b / 256 from there on
static int bt_range_t(int64_t b) { return b < 2048 ? 128 : BT_RANGE_MAX; }        // rows per workgroup
static int bt_wcols_t(int64_t b) { return b < 2048 ? 8 : 16; }                    // columns per wave, four waves per tile

// a lane's 16 B of one column of the range, rows ii (and ii + 1): zero beyond the n rows of the range
__device__ __forceinline__ cplx bt_ld_rows(const cplx* p, int ii, int n) { return ii < n ? *p : make_double2(0.0, 0.0); }
__device__ __forceinline__ f4u bt_ld_rows(const cplx32* p, int ii, int n) {
    f4u v = {0.f, 0.f, 0.f, 0.f};
    if (ii + 1 < n) v = *(const f4u*)p;
    else if (ii < n) { const cplx32 e = *p; v.x = e.x; v.y = e.y; }          // the last row of an odd plane
    return v;
}

template <int R, typename T>
__global__ __launch_bounds__(64 * BT_WAVES) void k_btb_product_t(const T* __restrict__ Sk, int64_t b, int wcols, int range, const cplx* __restrict__ t,
                                                                 cplx* __restrict__ part) {
    constexpr int LR = BT_LANE_ROWS<T>;
    constexpr int NCH = BT_RANGE_MAX / (64 * LR);                             // lane loads per column and range at most: 4, or 2 of float pairs
    constexpr int CJ = BT_CJ * LR;                                            // columns in flight: 2, or 4 of float pairs (8 loads either way)
    constexpr int P = bt_pow2(2 * CJ * R);
    using V = decltype(bt_ld_rows((const T*)nullptr, 0, 0));
    __shared__ cplx ts[BT_RANGE_MAX * R];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i0 = (int64_t)blockIdx.y * range;
    const int n = (int)(b - i0 < range ? b - i0 : range);
    // t of the range, member by member, zero beyond its n rows: the loop below multiplies whole lane loads
    for (int e = threadIdx.x; e < BT_RANGE_MAX * R; e += 64 * BT_WAVES)
        ts[(e % R) * BT_RANGE_MAX + e / R] = e < n * R ? t[i0 * R + e] : make_double2(0.0, 0.0);
    __syncthreads();
    const int64_t jw = ((int64_t)blockIdx.x * BT_WAVES + wave) * wcols;
    for (int cg = 0; cg < wcols && jw + cg < b; cg += CJ) {                   // (uniform over the wave; no barrier below)
        const int64_t j = jw + cg;
        const int ncj = (int)(b - j < CJ ? b - j : CJ);
        // every load of the pass first: NCH x CJ = 8 of 16 B per lane in flight.  A column past the plane repeats column j, unused.
        V sv[NCH][CJ];
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
            for (int c = 0; c < CJ; ++c) {
                const int ii = (ch * 64 + lane) * LR;
                sv[ch][c] = bt_ld_rows(Sk + i0 + ii + (j + (c < ncj ? c : 0)) * b, ii, n);
            }
        cplx acc[CJ][R];
#pragma unroll
        for (int c = 0; c < CJ; ++c)
#pragma unroll
            for (int r = 0; r < R; ++r) acc[c][r] = make_double2(0.0, 0.0);
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            if (ch * 64 * LR >= n) break;                                     // (uniform)
            const int ii = (ch * 64 + lane) * LR;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const cplx t0 = ts[r * BT_RANGE_MAX + ii];
                if constexpr (LR == 2) {
                    const cplx t1 = ts[r * BT_RANGE_MAX + ii + 1];
#pragma unroll
                    for (int c = 0; c < CJ; ++c) {
                        cfma_x(acc[c][r], make_double2((double)sv[ch][c].x, (double)sv[ch][c].y), t0);
                        cfma_x(acc[c][r], make_double2((double)sv[ch][c].z, (double)sv[ch][c].w), t1);
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < CJ; ++c) cfma_x(acc[c][r], sv[ch][c], t0);
                }
            }
        }
        double v[P];
#pragma unroll
        for (int q = 0; q < P; ++q) v[q] = 0.0;
#pragma unroll
        for (int c = 0; c < CJ; ++c)
#pragma unroll
            for (int r = 0; r < R; ++r) { v[2 * (c * R + r)] = acc[c][r].x; v[2 * (c * R + r) + 1] = acc[c][r].y; }
        bt_wave_sums(v);
        const int idx = bt_scatter_index<P>(lane), c = idx / (2 * R), r = (idx / 2) % R;
        if ((lane & BT_HOLDER_MASK<P>) == 0 && c < ncj)
            ((double*)&part[((int64_t)blockIdx.y * R + r) * b + j + c])[idx & 1] = v[0];
    }
}

// the column ranges in range order: forward writes (z_r)_k, backward updates it in place to (x_r)_k
template <bool FWD>
__global__ __launch_bounds__(256) void k_btb_fold(int64_t b, int k, int R, int nranges, int64_t N, const cplx* __restrict__ part, cplx* __restrict__ x) {
    const int64_t idx = blockIdx.x * (int64_t)256 + threadIdx.x;
    if (idx >= b * R) return;
    const int64_t i = idx % b, r = idx / b;
    cplx s = make_double2(0.0, 0.0);
    for (int c = 0; c < nranges; ++c) { const cplx v = part[((int64_t)c * R + r) * b + i]; s.x += v.x; s.y += v.y; }
    cplx& o = x[r * N + (int64_t)k * b + i];
    if (FWD) o = s; else { o.x -= s.x; o.y -= s.y; }
}

// ---- host side -----------------------------------------------------------------------------------------------------

// the stored inverses under their own type: f(S) with S the float pairs or the complex doubles; stored_t<decltype(S)> is T
template <class F> static void with_storage(const BlockTri* bt, F&& f) {
    if (bt->prec == BLOCKTRI_INV_F32) f((const cplx32*)bt->S32.p); else f((const cplx*)bt->S.p);
}
template <class P> using stored_t = std::remove_const_t<std::remove_pointer_t<P>>;

// the order of the two sweeps: forward k = 0 .. K-1, then backward k = K-2 .. 0; f(k, true_type) / f(k, false_type)
template <class F> static void each_step(int64_t K, F&& f) {
    for (int k = 0; k < (int)K; ++k) f(k, std::true_type{});
    for (int k = (int)K - 2; k >= 0; --k) f(k, std::false_type{});
}

int blocktri_sweep_launches(const BlockTri* bt) { return bt->b <= WALK_B ? 1 : (int)(2 * bt->K - 1); }

void blocktri_enqueue(const BlockTri* bt, const cplx* w, cplx* x, hipStream_t st, bool transposed) {
    LSFC_REQUIRE(!transposed || bt->has_t, "internal: transposed sweep without its tables");
    const BtApply a = bt->tables(transposed);
    const dim3 wg(AP_ROWS * AP_SLOTS);
    with_storage(bt, [&](auto S) {
        using T = stored_t<decltype(S)>;
        if (bt->b <= WALK_B) {
            if (transposed) hipLaunchKernelGGL(k_bt_walk_t<T>, dim3(1), wg, 0, st, a, S, w, x);
            else hipLaunchKernelGGL(k_bt_walk<T>, dim3(1), wg, 0, st, a, S, w, x);
            return;
        }
        const dim3 g(nblk(bt->b, transposed ? ST_COLS : AP_ROWS * BT_LANE_ROWS<T>));
        each_step(bt->K, [&](int k, auto fwd) {
            constexpr bool FWD = decltype(fwd)::value;
            if (transposed) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bt_step_t<FWD, T>), g, wg, 0, st, a, S, k, w, x);
            else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bt_step<FWD, T>), g, wg, 0, st, a, S, k, w, x);
        });
    });
}

int64_t blocktri_batch_reserve(BlockTri* bt, int R) {
    if (R > bt->batch_cap) {
        const int64_t nranges = std::max<int64_t>(nblk(bt->b, bb_cols(bt->b)), nblk(bt->b, bt_range_t(bt->b)));   // either sweep
        bt->bt_t.alloc((size_t)(bt->b * R)); bt->bt_part.alloc((size_t)(nranges * R * bt->b));
        bt->batch_cap = R;
    }
    return (int64_t)(bt->bt_t.bytes() + bt->bt_part.bytes());
}

void blocktri_enqueue_batch(const BlockTri* bt, int R, const cplx* w, cplx* x, hipStream_t st, bool transposed) {
    LSFC_REQUIRE(R >= 1 && R <= 8 && R <= bt->batch_cap, "internal: group of %d right-hand sides, work space for %d", R, bt->batch_cap);
    LSFC_REQUIRE(!transposed || bt->has_t, "internal: transposed sweep without its tables");
    const BtApply a = bt->tables(transposed);
    const int64_t b = bt->b, N = bt->N;
    const int cols = bb_cols(b), range = bt_range_t(b), wcols = bt_wcols_t(b), nranges = (int)nblk(b, transposed ? range : cols);
    const unsigned g = nblk(b * R, 256);
    cplx* t = bt->bt_t.p; cplx* part = bt->bt_part.p;
    with_storage(bt, [&](auto S) { dispatch<1, 8>(R, "block-tridiagonal group apply", [&](auto rc) {
        using T = stored_t<decltype(S)>;
        const dim3 pg(nblk(b, BB_ROWS * BT_LANE_ROWS<T>), (unsigned)nranges), pgt(nblk(b, BT_WAVES * wcols), (unsigned)nranges);
        each_step(bt->K, [&](int k, auto fwd) {
            constexpr bool FWD = decltype(fwd)::value;
            hipLaunchKernelGGL(k_btb_stage<FWD>, dim3(g), dim3(256), 0, st, a, k, R, N, w, (const cplx*)x, t);
            if (transposed)
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_btb_product_t<decltype(rc)::value, T>), pgt, dim3(64 * BT_WAVES), 0, st, S + (int64_t)k * b * b, b, wcols,
                                   range, (const cplx*)t, part);
            else
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_btb_product<decltype(rc)::value, T>), pg, dim3(BB_ROWS * BB_SLOTS), 0, st, S + (int64_t)k * b * b, b, cols,
                                   (const cplx*)t, part);
            hipLaunchKernelGGL(k_btb_fold<FWD>, dim3(g), dim3(256), 0, st, b, k, R, nranges, N, (const cplx*)part, x);
        });
    }); });
}

__global__ void k_warmup_blocktri_sweep(int* p) { if (p) *p = 0; }
void warmup_blocktri_sweep() {
    hipLaunchKernelGGL(k_warmup_blocktri_sweep, dim3(1), dim3(64), 0, 0, (int*)nullptr);
    LSFC_HIP(hipGetLastError());
}

} // namespace lsfc
