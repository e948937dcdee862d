// Factorisation of Msp on the device and the apply of Msp^{-1} from it.
//
// As, AG and Msp of the sparsifying preconditioner (src/preconditioner.jl:27-58; examples/example3D.jl:57-68) carry the
// full 9-point / 27-point stencil of an n x m (x l) grid, x fastest.  With the slowest axis as block index Msp is
// block tridiagonal: K blocks of b = N / K rows, diagonal blocks D_k, couplings L_k (block k to k-1), U_k (k to k+1).
// Exact block elimination
//     S_0 = D_0,   S_k = D_k - L_k S_{k-1}^{-1} U_{k-1}
//     forward   z_k = S_k^{-1} (w_k - L_k z_{k-1})
//     backward  x_{K-1} = z_{K-1},   x_k = z_k - S_k^{-1} (U_k x_{k+1})
// with the explicit inverses S_k^{-1} stored dense (column-major, K b^2 16 B).  The reference has UMFPACK's lu(Msp) here.
//
// Storage of the inverses: complex double, or (LSFC_PRECOND_INV_F32) interleaved float pairs, K b^2 8 B.  The elimination
// is the same fp64 arithmetic either way: at float storage block k is inverted in one of two fp64 work blocks (the Schur
// update of block k + 1 reads it there), then rounded once to nearest-even into the float array.  The sweeps widen every
// stored entry to fp64 on load and sum in fp64 in the order of the fp64 object.  There is one sweep kernel per shape, a
// template over the stored type T (k_bt_walk<T>, k_bt_step<FWD, T>, k_btb_product<R, T>), and the enqueue functions pick
// T once (with_storage).  The storages differ in the load alone: a lane's 16 B load is one row of complex double, or
// rows i and i + 1 of float pairs (BT_LANE_ROWS<T>; bt_accum / bt_accum2 in the step, the column loop in the product),
// so a workgroup covers twice the rows at float storage.  Staging, chunk loop, accumulators, LDS fold and store are shared.
//
// Set-up, per block:  Schur update as two sparse gathers (W = L_k S_{k-1}^{-1}; S_k = D_k - W U_{k-1}, U by columns),
// then a blocked in-place Gauss-Jordan inversion without pivoting, panels of 32 columns:
//     P = A_JJ^{-1}                       one workgroup, in LDS; |pivot| / max|S_k| is monitored
//     A_J: <- P A_J:,  A_:J <- -A_:J P    panel kernels (VALU), the old column panel and the new row panel are kept aside
//     A_ij <- A_ij - A_iJ(old) A_Jj(new)  the trailing update: complex fp64 GEMM on v_mfma_f64_16x16x4_f64
// No float atomics anywhere and every sum in a fixed order: two factorisations of one input are bitwise equal.
//
// Partial row pivoting inside a Schur block (BLOCKTRI_PIVOT_PARTIAL): before the three kernels of a step, one workgroup
// factorises a scratch copy of the tall panel (rows j0 .. b-1) by LU with row interchanges -- rows >= p of column p are the
// same in Gauss-Jordan and in LU at step p -- and composes the panel's interchanges into one list of row moves; a second
// kernel applies the moves to whole rows of the block.  The step then runs on the permuted block as it stands.  After the
// last panel the block is (Pi S_k)^{-1}; its columns are put back once through W, so that S_k^{-1} itself is stored and
// nothing after the inversion knows of the pivoting.
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
#include "blocktri.hpp"
#include <algorithm>
#include <chrono>
#include <memory>
#include <vector>

namespace lsfc {

static constexpr int NB = 32;             // panel width of the inversion = tile edge of the trailing update
static constexpr int AP_ROWS = 16;        // apply: rows of S_k^{-1} per workgroup ...
static constexpr int AP_SLOTS = 32;       // ... times column slots = 512 threads
static constexpr int AP_CHUNK = 2048;     // apply: entries of the stencil product staged in LDS at a time
static constexpr int WALK_B = 96;         // planes of at most this many rows: both sweeps inside one launch

struct BtStatus { int bad_block, bad_row; double bad_ratio, min_ratio, smax; int bad_band, bad_format; };

__device__ __forceinline__ cplx cmul(cplx a, cplx b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ void cfma(cplx& s, cplx a, cplx b) { s.x += a.x * b.x - a.y * b.y; s.y += a.x * b.y + a.y * b.x; }

// ---- set-up: pattern ---------------------------------------------------------------------------------------------

// one thread per row: checks the row (columns ascending, in range, inside the three block diagonals), splits it at the
// block boundaries (rlo: first entry of the diagonal block, rhi: first entry of the upper coupling), narrows the columns
// to 32 bits and counts the entries of the upper couplings per column
__global__ void k_bt_check(int64_t N, int64_t b, int64_t nnz, const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col,
                           int64_t* __restrict__ rlo, int64_t* __restrict__ rhi, int* __restrict__ col32, int* __restrict__ ucnt, BtStatus* st) {
    const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (r >= N) return;
    const int64_t s = rowptr[r], e = rowptr[r + 1], k = r / b;
    if (s < 0 || e < s || e > nnz) { atomicMin(&st->bad_format, (int)r); return; }
    int64_t prev = -1, lo = e, hi = e;
    bool fmt = true, band = true;
    for (int64_t q = s; q < e; ++q) {
        const int64_t c = col[q];
        if (c <= prev || c >= N) { fmt = false; break; }
        prev = c;
        const int64_t cb = c / b;
        if (cb < k - 1 || cb > k + 1) { band = false; continue; }
        if (cb >= k && lo == e) lo = q;
        if (cb > k && hi == e) hi = q;
        col32[q] = (int)c;
    }
    if (!fmt) { atomicMin(&st->bad_format, (int)r); return; }
    if (!band) { atomicMin(&st->bad_band, (int)r); return; }
    if (lo > hi) lo = hi;                                  // no entry in the diagonal block
    rlo[r] = lo; rhi[r] = hi;
    for (int64_t q = hi; q < e; ++q) atomicAdd(&ucnt[col32[q]], 1);
}

// upper couplings by columns: slots handed out by an integer counter, then every column sorted by row, so the result
// does not depend on the order in which the counter was served
__global__ void k_bt_ufill(int64_t N, const int64_t* __restrict__ rowptr, const int64_t* __restrict__ rhi, const int* __restrict__ col32,
                           const int64_t* __restrict__ ucolptr, int* __restrict__ ucur, int* __restrict__ urow, int64_t* __restrict__ uidx) {
    const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (r >= N) return;
    for (int64_t q = rhi[r]; q < rowptr[r + 1]; ++q) {
        const int c = col32[q];
        const int64_t at = ucolptr[c] + atomicAdd(&ucur[c], 1);
        urow[at] = (int)r; uidx[at] = q;
    }
}

__global__ void k_bt_usort(int64_t N, const int64_t* __restrict__ ucolptr, int* __restrict__ urow, int64_t* __restrict__ uidx,
                           const cplx* __restrict__ val, cplx* __restrict__ uval) {
    const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (c >= N) return;
    const int64_t s = ucolptr[c], e = ucolptr[c + 1];
    for (int64_t i = s + 1; i < e; ++i) {                  // insertion sort: a column holds a handful of entries
        const int r = urow[i]; const int64_t x = uidx[i];
        int64_t j = i;
        while (j > s && urow[j - 1] > r) { urow[j] = urow[j - 1]; uidx[j] = uidx[j - 1]; --j; }
        urow[j] = r; uidx[j] = x;
    }
    for (int64_t i = s; i < e; ++i) uval[i] = val[uidx[i]];
}

// The transposed tables (blocktri_transpose_tables) are one more transposition by the same two kernels -- k_bt_ufill from
// rowptr[r] instead of rhi[r] takes the whole row, k_bt_usort sorts every row of the transpose by its column -- with the
// count of all entries per column before it and the split of the transposed rows after it.
__global__ void k_bt_tcount(int64_t nnz, const int* __restrict__ col32, int* __restrict__ cnt) {
    const int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (q < nnz) atomicAdd(&cnt[col32[q]], 1);
}

// row c of the transpose: where its diagonal block and its upper coupling begin (as k_bt_check splits a row of Msp), and the
// values of As^T on the transposed pattern
__global__ void k_bt_tsplit(int64_t N, int64_t b, const int64_t* __restrict__ tptr, const int* __restrict__ tcol, const int64_t* __restrict__ tidx,
                            const cplx* __restrict__ as_val, int64_t* __restrict__ rlo, int64_t* __restrict__ rhi, cplx* __restrict__ tas) {
    const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (c >= N) return;
    const int64_t s = tptr[c], e = tptr[c + 1], k = c / b;
    int64_t lo = e, hi = e;
    for (int64_t q = s; q < e; ++q) {
        const int64_t cb = tcol[q] / b;
        if (cb >= k && lo == e) lo = q;
        if (cb > k && hi == e) hi = q;
        tas[q] = as_val[tidx[q]];
    }
    if (lo > hi) lo = hi;
    rlo[c] = lo; rhi[c] = hi;
}

// ---- set-up: Schur update ------------------------------------------------------------------------------------------

// W = L_k S_{k-1}^{-1}: W[i, r] = sum over the lower coupling of row i
__global__ void k_bt_schur_left(int64_t b, int64_t k, const int64_t* __restrict__ rowptr, const int64_t* __restrict__ rlo, const int* __restrict__ col32,
                                const cplx* __restrict__ val, const cplx* __restrict__ Sprev, cplx* __restrict__ W) {
    const int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (idx >= b * b) return;
    const int64_t i = idx % b, r = idx / b, g = k * b + i, base = (k - 1) * b;
    cplx s = make_double2(0.0, 0.0);
    for (int64_t q = rowptr[g]; q < rlo[g]; ++q) cfma(s, val[q], Sprev[(col32[q] - base) + r * b]);
    W[idx] = s;
}

// S = -W U_{k-1}: S[i, j] = -sum over column j of the upper coupling of block k-1
__global__ void k_bt_schur_right(int64_t b, int64_t k, const int64_t* __restrict__ ucolptr, const int* __restrict__ urow, const cplx* __restrict__ uval,
                                 const cplx* __restrict__ W, cplx* __restrict__ S) {
    const int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (idx >= b * b) return;
    const int64_t i = idx % b, j = idx / b, g = k * b + j, base = (k - 1) * b;
    cplx s = make_double2(0.0, 0.0);
    for (int64_t q = ucolptr[g]; q < ucolptr[g + 1]; ++q) cfma(s, W[i + (urow[q] - base) * b], uval[q]);
    S[idx] = make_double2(-s.x, -s.y);
}

// S += D_k (every stored entry of the diagonal block once: columns are strictly ascending)
__global__ void k_bt_add_diag(int64_t b, int64_t k, const int64_t* __restrict__ rlo, const int64_t* __restrict__ rhi, const int* __restrict__ col32,
                              const cplx* __restrict__ val, cplx* __restrict__ S) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= b) return;
    const int64_t g = k * b + i;
    for (int64_t q = rlo[g]; q < rhi[g]; ++q) {
        cplx& d = S[i + (col32[q] - k * b) * b];
        d.x += val[q].x; d.y += val[q].y;
    }
}

// max |S_ij|^2 in two steps (a maximum does not depend on the order)
__global__ __launch_bounds__(256) void k_bt_absmax_part(int64_t n, const cplx* __restrict__ S, double* __restrict__ part) {
    __shared__ double red[256];
    double m = 0.0;
    for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) { const cplx v = S[i]; m = fmax(m, v.x * v.x + v.y * v.y); }
    red[threadIdx.x] = m;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + o]); __syncthreads(); }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}
__global__ __launch_bounds__(256) void k_bt_absmax_fin(int nparts, const double* __restrict__ part, BtStatus* st) {
    __shared__ double red[256];
    red[threadIdx.x] = (int)threadIdx.x < nparts ? part[threadIdx.x] : 0.0;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + o]); __syncthreads(); }
    if (threadIdx.x == 0) st->smax = sqrt(red[0]);
}

// ---- set-up: blocked Gauss-Jordan inversion, in place, no pivoting ------------------------------------------------

// P = A_JJ^{-1} (nb x nb, nb <= 32) by one workgroup of 32 x 32 threads, thread (r, c) owns one entry in LDS.
// Monitor: |pivot| / max|S_k|; the first pivot below `thr` (or not a number) is recorded with block and row.
__global__ __launch_bounds__(1024) void k_bt_diag(const cplx* __restrict__ A, int64_t b, int j0, int nb, cplx* __restrict__ P, BtStatus* st,
                                                  int block, double thr) {
    __shared__ cplx M[NB][NB + 1];
    const int c = threadIdx.x & 31, r = threadIdx.x >> 5;
    M[r][c] = (r < nb && c < nb) ? A[(j0 + r) + (int64_t)(j0 + c) * b] : make_double2(r == c ? 1.0 : 0.0, 0.0);
    __syncthreads();
    const double smax = st->smax;
    double minr = 1e300, badr = 0.0; int bad = -1;
    for (int p = 0; p < nb; ++p) {
        const cplx piv = M[p][p], f = M[r][p], v = M[r][c], rp = M[p][c];
        __syncthreads();
        const double a2 = piv.x * piv.x + piv.y * piv.y;
        const double ratio = sqrt(a2) / smax;
        if (!(ratio >= thr) && bad < 0) { bad = p; badr = ratio; }
        if (ratio < minr) minr = ratio;
        const cplx ip = make_double2(piv.x / a2, -piv.y / a2);
        const cplx sp = c == p ? ip : cmul(rp, ip);                          // row p of the step's result
        cplx nv;
        if (r == p) nv = sp;
        else { const cplx t = cmul(f, sp); nv = c == p ? make_double2(-t.x, -t.y) : make_double2(v.x - t.x, v.y - t.y); }
        M[r][c] = nv;
        __syncthreads();
    }
    P[r + c * NB] = M[r][c];
    if (threadIdx.x == 0) {
        if (minr < st->min_ratio) st->min_ratio = minr;
        if (bad >= 0 && st->bad_block < 0) { st->bad_block = block; st->bad_row = j0 + bad; st->bad_ratio = badr; }
    }
}

// Both panels of one step.  Workgroups [0, nx): the row panel, a thread per column j outside J: A_Jj <- P A_Jj, kept
// aside in R (32 x b, rows beyond nb zero).  Workgroups [nx, 2 nx): the column panel, a thread per row i outside J:
// C_i <- A_iJ (b x 32, columns beyond nb zero), A_iJ <- -A_iJ P; rows inside J: A_JJ <- P.
__global__ __launch_bounds__(256) void k_bt_panels(cplx* __restrict__ A, int64_t b, int j0, int nb, const cplx* __restrict__ P,
                                                   cplx* __restrict__ R, cplx* __restrict__ Cb, int nx) {
    __shared__ cplx Ps[NB][NB + 1];                                         // Ps[r][c] = P[r, c]
    for (int t = threadIdx.x; t < NB * NB; t += 256) Ps[t % NB][t / NB] = P[t];
    __syncthreads();
    const bool rowpart = (int)blockIdx.x < nx;
    const int64_t t = (int64_t)(rowpart ? blockIdx.x : blockIdx.x - nx) * 256 + threadIdx.x;
    if (t >= b) return;
    const bool inJ = t >= j0 && t < j0 + nb;
    cplx a[NB];
    if (rowpart) {
        if (inJ) return;
#pragma unroll
        for (int c = 0; c < NB; ++c) a[c] = c < nb ? A[(j0 + c) + t * b] : make_double2(0.0, 0.0);
        for (int r = 0; r < NB; ++r) {
            cplx s = make_double2(0.0, 0.0);
            if (r < nb) {
#pragma unroll
                for (int c = 0; c < NB; ++c) cfma(s, Ps[r][c], a[c]);
                A[(j0 + r) + t * b] = s;
            }
            R[r + t * NB] = s;
        }
    } else {
        if (inJ) {
            for (int c = 0; c < NB; ++c) { Cb[t + (int64_t)c * b] = make_double2(0.0, 0.0); if (c < nb) A[t + (int64_t)(j0 + c) * b] = Ps[t - j0][c]; }
            return;
        }
#pragma unroll
        for (int c = 0; c < NB; ++c) { a[c] = c < nb ? A[t + (int64_t)(j0 + c) * b] : make_double2(0.0, 0.0); Cb[t + (int64_t)c * b] = a[c]; }
        for (int c = 0; c < nb; ++c) {
            cplx s = make_double2(0.0, 0.0);
#pragma unroll
            for (int q = 0; q < NB; ++q) cfma(s, a[q], Ps[q][c]);             // (rows q >= nb of a are zero)
            A[t + (int64_t)(j0 + c) * b] = make_double2(-s.x, -s.y);
        }
    }
}

// Trailing update A_ij <- A_ij - C_i R_j over all 32 x 32 tiles outside panel row / panel column J: one wave per tile,
// 2 x 2 MFMA tiles of 16 x 16, each complex product as four real v_mfma_f64_16x16x4_f64.  The product is formed
// transposed (MFMA rows = matrix columns j, MFMA columns = matrix rows i) so that the 16 lanes of a result register
// sit on 16 consecutive rows of the column-major matrix: 256 B per access.
// Lane maps (cdna_hip_programming.md): A operand [row = lane & 15][k = lane >> 4], B operand [k = lane >> 4][col = lane & 15],
// result register g: [row = (lane >> 4) + 4 g][col = lane & 15].
typedef double d4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void k_bt_trail(cplx* __restrict__ A, int64_t b, int J, int nt, const cplx* __restrict__ R, const cplx* __restrict__ Cb) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= (int64_t)nt * nt) return;                                      // (whole waves leave together)
    const int ti = (int)(w % nt), tj = (int)(w / nt);
    if (ti == J || tj == J) return;
    const int c16 = lane & 15, q = lane >> 4;
    d4 re[2][2], im[2][2];                                                  // [sj][si]
#pragma unroll
    for (int sj = 0; sj < 2; ++sj)
#pragma unroll
        for (int si = 0; si < 2; ++si) {
            const int64_t i = (int64_t)ti * NB + si * 16 + c16;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int64_t j = (int64_t)tj * NB + sj * 16 + q + 4 * g;
                const cplx v = (i < b && j < b) ? A[i + j * b] : make_double2(0.0, 0.0);
                re[sj][si][g] = v.x; im[sj][si][g] = v.y;
            }
        }
#pragma unroll
    for (int k0 = 0; k0 < NB; k0 += 4) {
        const int kk = k0 + q;
        cplx cn[2], rv[2];
#pragma unroll
        for (int si = 0; si < 2; ++si) {
            const int64_t i = (int64_t)ti * NB + si * 16 + c16;
            const cplx v = i < b ? Cb[i + (int64_t)kk * b] : make_double2(0.0, 0.0);
            cn[si] = make_double2(-v.x, -v.y);
        }
#pragma unroll
        for (int sj = 0; sj < 2; ++sj) {
            const int64_t j = (int64_t)tj * NB + sj * 16 + c16;
            rv[sj] = j < b ? R[kk + j * NB] : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int sj = 0; sj < 2; ++sj)
#pragma unroll
            for (int si = 0; si < 2; ++si) {
                re[sj][si] = __builtin_amdgcn_mfma_f64_16x16x4f64(rv[sj].x, cn[si].x, re[sj][si], 0, 0, 0);
                re[sj][si] = __builtin_amdgcn_mfma_f64_16x16x4f64(-rv[sj].y, cn[si].y, re[sj][si], 0, 0, 0);
                im[sj][si] = __builtin_amdgcn_mfma_f64_16x16x4f64(rv[sj].x, cn[si].y, im[sj][si], 0, 0, 0);
                im[sj][si] = __builtin_amdgcn_mfma_f64_16x16x4f64(rv[sj].y, cn[si].x, im[sj][si], 0, 0, 0);
            }
    }
#pragma unroll
    for (int sj = 0; sj < 2; ++sj)
#pragma unroll
        for (int si = 0; si < 2; ++si) {
            const int64_t i = (int64_t)ti * NB + si * 16 + c16;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int64_t j = (int64_t)tj * NB + sj * 16 + q + 4 * g;
                if (i < b && j < b) A[i + j * b] = make_double2(re[sj][si][g], im[sj][si][g]);
            }
        }
}

// ---- set-up: partial row pivoting ------------------------------------------------------------------------------------

static constexpr int PV_THREADS = 1024;   // the panel factorisation: one workgroup, thread t owns rows t, t + 1024, ...
static constexpr int PV_MOVES = 2 * NB;   // rows that the interchanges of one panel can touch

// (|v|^2, row) of a pivot candidate: the larger modulus wins, on a tie the lower row (a total order, so the result does
// not depend on the order in which candidates are compared); a modulus that is not a number never wins
__device__ __forceinline__ void pv_better(double& bm, int& bi, double m, int i) { if (m > bm || (m == bm && i < bi)) { bm = m; bi = i; } }
__device__ __forceinline__ double pv_abs2(cplx v) { return __dadd_rn(__dmul_rn(v.x, v.x), __dmul_rn(v.y, v.y)); }

// The pivots of panel J = [j0, j0 + nb): LU with partial pivoting of the tall panel A[j0 .. b-1, J] on the scratch copy T
// (h = b - j0 rows, leading dimension b), with the arithmetic of k_bt_diag, by ONE workgroup.  A thread keeps its rows
// for the whole panel, so per step only the two interchanged rows pass between threads: two barriers per step.  The
// modulus of the next column is taken while that column is updated.  Thread 0 composes the interchanges: mpos / mval is
// a map "position -> row now there" over the <= 64 positions touched.  Out: nmoves and moves[2 i] = position,
// moves[2 i + 1] = row that goes there (both relative to j0, only where they differ); perm (b entries of this block,
// perm[i] = row of S_k now at position i) is set to the identity by the first panel and updated by every panel.
__global__ __launch_bounds__(PV_THREADS) void k_bt_pivot_panel(const cplx* __restrict__ A, int64_t b, int j0, int nb, cplx* T,
                                                               int* __restrict__ moves, int* perm) {
    __shared__ double rm[PV_THREADS / 64]; __shared__ int ri[PV_THREADS / 64];
    __shared__ cplx prow[NB];
    __shared__ int mpos[PV_MOVES], mval[PV_MOVES], mcnt, oldp[PV_MOVES];
    const int tid = threadIdx.x, h = (int)(b - j0);
    if (j0 == 0) for (int i = tid; i < h; i += PV_THREADS) perm[i] = i;
    if (tid == 0) mcnt = 0;
    double bm = -1.0; int bi = 0;
    for (int i = tid; i < h; i += PV_THREADS) {
        for (int c = 0; c < nb; ++c) {
            const cplx v = A[(j0 + i) + (int64_t)(j0 + c) * b];
            T[i + (int64_t)c * b] = v;
            if (c == 0) pv_better(bm, bi, pv_abs2(v), i);
        }
    }
    for (int p = 0; p < nb; ++p) {
        // the pivot of column p among rows p .. h-1: lanes, then waves (every thread folds the 16 wave results itself)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const double m = __shfl_xor(bm, o, 64); const int i = __shfl_xor(bi, o, 64); pv_better(bm, bi, m, i); }
        if ((tid & 63) == 0) { rm[tid >> 6] = bm; ri[tid >> 6] = bi; }
        __syncthreads();
        double qm = -1.0; int q = p;
        for (int w = 0; w < PV_THREADS / 64; ++w) pv_better(qm, q, rm[w], ri[w]);
        if (qm < 0.0) q = p;                                                 // no candidate is a number: k_bt_diag reports the pivot
        if (tid < nb) {                                                      // interchange rows p and q of T; the new row p aside
            const cplx vq = T[q + (int64_t)tid * b];
            if (q != p) { T[q + (int64_t)tid * b] = T[p + (int64_t)tid * b]; T[p + (int64_t)tid * b] = vq; }
            prow[tid] = vq;
        }
        if (tid == 0 && q != p) {
            int ip = -1, iq = -1;
            for (int e = 0; e < mcnt; ++e) { if (mpos[e] == p) ip = e; if (mpos[e] == q) iq = e; }
            if (ip < 0) { ip = mcnt++; mpos[ip] = p; mval[ip] = p; }
            if (iq < 0) { iq = mcnt++; mpos[iq] = q; mval[iq] = q; }
            const int t = mval[ip]; mval[ip] = mval[iq]; mval[iq] = t;
        }
        __syncthreads();
        bm = -1.0; bi = 0;
        if (p + 1 < nb) {
            const cplx piv = prow[p];
            const double a2 = piv.x * piv.x + piv.y * piv.y;
            const cplx ip = make_double2(piv.x / a2, -piv.y / a2);
            for (int i = tid; i < h; i += PV_THREADS) {
                if (i <= p) continue;
                const cplx f = T[i + (int64_t)p * b];
                for (int c = p + 1; c < nb; ++c) {
                    const cplx t = cmul(f, cmul(prow[c], ip)), v = T[i + (int64_t)c * b];
                    const cplx nv = make_double2(v.x - t.x, v.y - t.y);
                    T[i + (int64_t)c * b] = nv;
                    if (c == p + 1) pv_better(bm, bi, pv_abs2(nv), i);
                }
            }
        }
    }
    // the moves of this panel, and perm after them
    const int n = mcnt;
    if (tid < PV_MOVES) oldp[tid] = tid < n ? perm[j0 + mval[tid]] : 0;
    __syncthreads();
    if (tid < n) perm[j0 + mpos[tid]] = oldp[tid];
    if (tid == 0) {
        int cnt = 0;
        for (int e = 0; e < n; ++e) if (mval[e] != mpos[e]) { moves[1 + 2 * cnt] = mpos[e]; moves[2 + 2 * cnt] = mval[e]; ++cnt; }
        moves[0] = cnt;
    }
}

// The moves of one panel applied to whole rows of the block: one wave per column, lane e reads the entry that goes to
// position moves[e] and writes it there after the whole wave has read (4 columns per workgroup; the rows of a panel's own
// positions are consecutive, so half of the stores of a wave fall into 512 consecutive bytes).
__global__ __launch_bounds__(256) void k_bt_swap_rows(cplx* __restrict__ A, int64_t b, int j0, const int* __restrict__ moves) {
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int n = moves[0];
    const bool on = lane < n && c < b;
    cplx v = make_double2(0.0, 0.0);
    int dst = 0;
    if (on) { dst = moves[1 + 2 * lane]; v = A[(j0 + moves[2 + 2 * lane]) + c * b]; }
    __syncthreads();
    if (on) A[(j0 + dst) + c * b] = v;
}

// columns back in place after the last panel: B = (Pi S)^{-1} in A, S^{-1} = B Pi, column perm[j] of S^{-1} = column j of B
__global__ __launch_bounds__(256) void k_bt_unscramble(int64_t b, const cplx* __restrict__ A, const int* __restrict__ perm, cplx* __restrict__ W) {
    const int64_t idx = blockIdx.x * (int64_t)256 + threadIdx.x;
    if (idx >= b * b) return;
    const int64_t i = idx % b, j = idx / b;
    W[i + (int64_t)perm[j] * b] = A[idx];
}

// ---- the apply -----------------------------------------------------------------------------------------------------

struct BtApply {                   // what the sweep kernels read
    int64_t b; int K;
    const int64_t* rowptr; const int64_t* rlo; const int64_t* rhi; const int* col; const cplx* val;
};

// a stored entry of S_k^{-1} as fp64: the float form is widened (exact), all arithmetic after it is fp64
typedef float2 cplx32;
typedef float f4u __attribute__((ext_vector_type(4), aligned(8)));           // two consecutive float pairs of one column
__device__ __forceinline__ cplx bt_ld(const cplx* p) { return *p; }
__device__ __forceinline__ cplx bt_ld(const cplx32* p) { const cplx32 v = *p; return make_double2((double)v.x, (double)v.y); }

// fp64 work block -> float storage, round to nearest even, once per block
__global__ __launch_bounds__(256) void k_bt_round(int64_t n, const cplx* __restrict__ A, cplx32* __restrict__ S32) {
    const int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
    if (i >= n) return;
    const cplx v = A[i];
    S32[i] = make_float2(__double2float_rn(v.x), __double2float_rn(v.y));
}

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

struct BlockTri {
    int64_t N = 0, K = 0, b = 0, nnz = 0;
    DevBuf<int64_t> rowptr, rlo, rhi; DevBuf<int> col; DevBuf<cplx> val;     // private CSR of Msp, split at the block boundaries
    int prec = BLOCKTRI_INV_F64;
    DevBuf<cplx> S;                                                          // S_k^{-1}, k = 0 .. K-1 (fp64 storage) ...
    DevBuf<cplx32> S32;                                                      // ... or the same blocks rounded to float pairs
    int64_t factor_us = 0; double min_ratio = 0.0;
    bool pivoted = false; DevBuf<int> perm;                                  // partial pivoting: perm[k b + i] = row of S_k that became pivot row i
    DevBuf<cplx> bt_t, bt_part; int batch_cap = 0;                           // group apply: stencil products (b x R), partial sums (ranges x R x b)
    // the transposed apply (blocktri_transpose_tables, on first use): CSR of Msp^T split at the block boundaries as the one
    // above is, and the values of As^T on the same pattern
    DevBuf<int64_t> t_rowptr, t_rlo, t_rhi; DevBuf<int> t_col; DevBuf<cplx> t_val, t_as; bool has_t = false;
    BtApply tables(bool transposed) const {
        if (transposed) return BtApply{b, (int)K, t_rowptr.p, t_rlo.p, t_rhi.p, t_col.p, t_val.p};
        return BtApply{b, (int)K, rowptr.p, rlo.p, rhi.p, col.p, val.p};
    }
    int launches() const { return b <= WALK_B ? 1 : (int)(2 * K - 1); }
};

static double entry_bytes(int prec) { return prec == BLOCKTRI_INV_F32 ? 8.0 : 16.0; }

static double work_bytes(int64_t N, int64_t K, int prec, int pivoting) {
    const double b = (double)(N / K);
    const double blocks = prec == BLOCKTRI_INV_F32 ? 2.0 * b * b * 16.0 : 0.0;    // float storage: current and previous block in fp64
    // pivoting (PARTIAL, and AUTO, which may come to it): the scratch copy of the tall panel, the pivots (K b 4 B), the moves
    const double pivot = pivoting == BLOCKTRI_PIVOT_NONE ? 0.0 : b * NB * 16.0 + 4.0 * (double)N + 4.0 * (1 + 2 * PV_MOVES);
    return blocks + b * b * 16.0 + 2.0 * b * NB * 16.0 + 64.0 * (double)N + pivot;   // W, the two panels, row tables and vectors
}

BlockTriNeed blocktri_memory_need(int64_t N, int64_t K, int prec, int pivoting) {
    const double b = (double)(N / K);
    return BlockTriNeed{(double)K * b * b * entry_bytes(prec), work_bytes(N, K, prec, pivoting)};
}

void blocktri_require_memory(int64_t N, int64_t K, double extra, const char* who, int prec, int pivoting) {
    const BlockTriNeed nd = blocktri_memory_need(N, K, prec, pivoting);
    const double factors = nd.inverse_bytes, need = factors + nd.work_bytes + extra;
    size_t free_b = 0, total_b = 0;
    LSFC_HIP(hipMemGetInfo(&free_b, &total_b));
    if (need > (double)free_b)
        fail(LSFC_ENOMEM, "%s: %lld blocks of %lld x %lld complex need %.3f GB for the inverses S_k^{-1} stored as %s (K b^2 %d B) and %.3f GB of "
             "work space, %.3f GB of device memory are free", who, (long long)K, (long long)(N / K), (long long)(N / K), factors / 1e9,
             prec == BLOCKTRI_INV_F32 ? "complex64" : "complex128", (int)entry_bytes(prec), (need - factors) / 1e9, (double)free_b / 1e9);
}

static inline unsigned nblk(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

// one factorisation, with partial pivoting in every block or without any.  `breakdown` (may be NULL): a pivot below the
// threshold sets it and returns no object instead of failing -- BLOCKTRI_PIVOT_AUTO then repeats with pivoting.
static BlockTri* factor_once(int64_t N, int64_t K, const int64_t* rowptr, const int64_t* col, const cplx* msp, int prec, bool pivot, bool* breakdown) {
    const auto t0 = std::chrono::steady_clock::now();
    const int64_t b = N / K;
    LSFC_REQUIRE(b * b < ((int64_t)1 << 40), "block-tridiagonal preconditioner: block size %lld out of range", (long long)b);
    hipStream_t st = nullptr;
    std::unique_ptr<BlockTri> bt(new BlockTri());
    bt->N = N; bt->K = K; bt->b = b; bt->prec = prec;
    int64_t nnz = 0;
    LSFC_HIP(hipMemcpy(&nnz, rowptr + N, sizeof nnz, hipMemcpyDeviceToHost));
    LSFC_REQUIRE(nnz >= 1 && nnz < ((int64_t)1 << 40), "block-tridiagonal preconditioner: rowptr[N] = %lld is not a plausible entry count", (long long)nnz);
    bt->nnz = nnz;
    // pattern: check, split, upper couplings by columns
    bt->rowptr.alloc((size_t)N + 1); bt->rlo.alloc((size_t)N); bt->rhi.alloc((size_t)N); bt->col.alloc((size_t)nnz); bt->val.alloc((size_t)nnz);
    LSFC_HIP(hipMemcpyAsync(bt->rowptr.p, rowptr, ((size_t)N + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    LSFC_HIP(hipMemcpyAsync(bt->val.p, msp, (size_t)nnz * sizeof(cplx), hipMemcpyDeviceToDevice, st));
    DevBuf<BtStatus> dstat; dstat.alloc(1);
    BtStatus hs{};
    hs.bad_block = -1; hs.bad_row = -1; hs.min_ratio = 1e300; hs.smax = 0.0; hs.bad_band = hs.bad_format = 0x7fffffff;
    LSFC_HIP(hipMemcpyAsync(dstat.p, &hs, sizeof hs, hipMemcpyHostToDevice, st));
    DevBuf<int> ucnt; ucnt.alloc((size_t)N);
    LSFC_HIP(hipMemsetAsync(ucnt.p, 0, ucnt.bytes(), st));
    hipLaunchKernelGGL(k_bt_check, dim3(nblk(N, 256)), dim3(256), 0, st, N, b, nnz, bt->rowptr.p, col, bt->rlo.p, bt->rhi.p, bt->col.p, ucnt.p, dstat.p);
    LSFC_HIP(hipGetLastError());
    std::vector<int> hcnt((size_t)N);
    LSFC_HIP(hipMemcpyAsync(hcnt.data(), ucnt.p, ucnt.bytes(), hipMemcpyDeviceToHost, st));
    LSFC_HIP(hipMemcpyAsync(&hs, dstat.p, sizeof hs, hipMemcpyDeviceToHost, st));
    LSFC_HIP(hipStreamSynchronize(st));
    LSFC_REQUIRE(hs.bad_format == 0x7fffffff, "block-tridiagonal preconditioner: row %d is not a CSR row with ascending columns in [0, N)", hs.bad_format);
    LSFC_REQUIRE(hs.bad_band == 0x7fffffff, "block-tridiagonal preconditioner: row %d (block %lld) has an entry outside the three block diagonals "
                 "of %lld blocks of %lld rows", hs.bad_band, (long long)(hs.bad_band / b), (long long)K, (long long)b);
    std::vector<int64_t> hptr((size_t)N + 1, 0);
    for (int64_t c = 0; c < N; ++c) hptr[(size_t)c + 1] = hptr[(size_t)c] + hcnt[(size_t)c];
    const int64_t nnzU = hptr[(size_t)N];
    DevBuf<int64_t> ucolptr, uidx; DevBuf<int> urow; DevBuf<cplx> uval;
    ucolptr.alloc((size_t)N + 1); uidx.alloc((size_t)nnzU); urow.alloc((size_t)nnzU); uval.alloc((size_t)nnzU);
    LSFC_HIP(hipMemcpyAsync(ucolptr.p, hptr.data(), hptr.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    LSFC_HIP(hipMemsetAsync(ucnt.p, 0, ucnt.bytes(), st));
    if (nnzU) {
        hipLaunchKernelGGL(k_bt_ufill, dim3(nblk(N, 256)), dim3(256), 0, st, N, bt->rowptr.p, bt->rhi.p, bt->col.p, ucolptr.p, ucnt.p, urow.p, uidx.p);
        LSFC_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_bt_usort, dim3(nblk(N, 256)), dim3(256), 0, st, N, ucolptr.p, urow.p, uidx.p, bt->val.p, uval.p);
        LSFC_HIP(hipGetLastError());
    }
    // the blocks
    const bool f32 = prec == BLOCKTRI_INV_F32;
    DevBuf<cplx> work[2];                                                   // float storage: block k is inverted in work[k & 1] ...
    if (f32) { bt->S32.alloc((size_t)(K * b * b)); work[0].alloc((size_t)(b * b)); if (K > 1) work[1].alloc((size_t)(b * b)); }
    else bt->S.alloc((size_t)(K * b * b));
    DevBuf<cplx> W, P, R, Cb; DevBuf<double> part;
    if (K > 1 || pivot) W.alloc((size_t)(b * b));                           // (pivoting: the columns go back in place through W)
    DevBuf<cplx> T; DevBuf<int> moves;
    if (pivot) { T.alloc((size_t)(b * NB)); moves.alloc(1 + 2 * PV_MOVES); bt->perm.alloc((size_t)N); bt->pivoted = true; }
    P.alloc(NB * NB); R.alloc((size_t)(NB * b)); Cb.alloc((size_t)(b * NB)); part.alloc(256);
    const int nt = (int)((b + NB - 1) / NB), nx = (int)nblk(b, 256);
    const unsigned ebl = nblk(b * b, 256);
    for (int64_t k = 0; k < K; ++k) {
        cplx* Sk = f32 ? work[k & 1].p : bt->S.p + k * b * b;
        const cplx* Sprev = f32 ? work[(k + 1) & 1].p : Sk - b * b;           // ... and block k + 1 reads it there: fp64 S_k^{-1} either way
        if (k == 0) LSFC_HIP(hipMemsetAsync(Sk, 0, (size_t)(b * b) * sizeof(cplx), st));
        else {
            hipLaunchKernelGGL(k_bt_schur_left, dim3(ebl), dim3(256), 0, st, b, k, bt->rowptr.p, bt->rlo.p, bt->col.p, bt->val.p, Sprev, W.p);
            hipLaunchKernelGGL(k_bt_schur_right, dim3(ebl), dim3(256), 0, st, b, k, ucolptr.p, urow.p, uval.p, W.p, Sk);
        }
        hipLaunchKernelGGL(k_bt_add_diag, dim3(nblk(b, 256)), dim3(256), 0, st, b, k, bt->rlo.p, bt->rhi.p, bt->col.p, bt->val.p, Sk);
        hipLaunchKernelGGL(k_bt_absmax_part, dim3(256), dim3(256), 0, st, b * b, Sk, part.p);
        hipLaunchKernelGGL(k_bt_absmax_fin, dim3(1), dim3(256), 0, st, 256, part.p, dstat.p);
        for (int J = 0; J < nt; ++J) {
            const int j0 = J * NB, nb = (int)std::min<int64_t>(NB, b - j0);
            if (pivot) {
                hipLaunchKernelGGL(k_bt_pivot_panel, dim3(1), dim3(PV_THREADS), 0, st, (const cplx*)Sk, b, j0, nb, T.p, moves.p, bt->perm.p + k * b);
                hipLaunchKernelGGL(k_bt_swap_rows, dim3(nblk(b, 4)), dim3(256), 0, st, Sk, b, j0, (const int*)moves.p);
            }
            hipLaunchKernelGGL(k_bt_diag, dim3(1), dim3(1024), 0, st, Sk, b, j0, nb, P.p, dstat.p, (int)k, BLOCKTRI_PIVOT_MIN);
            hipLaunchKernelGGL(k_bt_panels, dim3(2 * nx), dim3(256), 0, st, Sk, b, j0, nb, P.p, R.p, Cb.p, nx);
            if (nt > 1) hipLaunchKernelGGL(k_bt_trail, dim3(nblk((int64_t)nt * nt, 4)), dim3(256), 0, st, Sk, b, J, nt, R.p, Cb.p);
        }
        if (pivot) {
            hipLaunchKernelGGL(k_bt_unscramble, dim3(ebl), dim3(256), 0, st, b, (const cplx*)Sk, (const int*)(bt->perm.p + k * b), W.p);
            LSFC_HIP(hipMemcpyAsync(Sk, W.p, (size_t)(b * b) * sizeof(cplx), hipMemcpyDeviceToDevice, st));
        }
        if (f32) hipLaunchKernelGGL(k_bt_round, dim3(ebl), dim3(256), 0, st, b * b, (const cplx*)Sk, bt->S32.p + k * b * b);
        LSFC_HIP(hipGetLastError());
    }
    LSFC_HIP(hipMemcpyAsync(&hs, dstat.p, sizeof hs, hipMemcpyDeviceToHost, st));
    LSFC_HIP(hipStreamSynchronize(st));
    if (hs.bad_block >= 0 && breakdown) { *breakdown = true; return nullptr; }
    if (pivot)
        LSFC_REQUIRE(hs.bad_block < 0, "block-tridiagonal preconditioner: breakdown in block %d at row %lld (pivot %d of the block): the largest candidate has "
                     "|pivot| / max|S_k| = %.3e, below %.1e -- the Schur block is singular to working precision (partial pivoting inside the block)",
                     hs.bad_block, (long long)(hs.bad_block * b + hs.bad_row), hs.bad_row, hs.bad_ratio, BLOCKTRI_PIVOT_MIN);
    LSFC_REQUIRE(hs.bad_block < 0, "block-tridiagonal preconditioner: breakdown in block %d at row %lld (row %d of the block): |pivot| / max|S_k| = %.3e is below %.1e "
                 "-- the Schur block is singular or needs pivoting; use the host LU route (lsfc_precond_create)", hs.bad_block,
                 (long long)(hs.bad_block * b + hs.bad_row), hs.bad_row, hs.bad_ratio, BLOCKTRI_PIVOT_MIN);
    bt->min_ratio = hs.min_ratio;
    bt->factor_us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    return bt.release();
}

BlockTri* blocktri_factor(int64_t N, int64_t K, const int64_t* rowptr, const int64_t* col, const cplx* msp, int prec, int pivoting) {
    if (pivoting != BLOCKTRI_PIVOT_AUTO) return factor_once(N, K, rowptr, col, msp, prec, pivoting == BLOCKTRI_PIVOT_PARTIAL, nullptr);
    bool breakdown = false;
    if (BlockTri* bt = factor_once(N, K, rowptr, col, msp, prec, false, &breakdown)) return bt;
    return factor_once(N, K, rowptr, col, msp, prec, true, nullptr);          // the whole factorisation again, pivoting in every block
}

// The tables of the transposed apply, built once: every entry (r, c) of the private CSR goes to row c of the transpose.
// Slots are handed out by integer counters and every transposed row is then sorted by its column, so two objects of one
// input hold the same tables.  Synchronous; allocates.
BlockTriT blocktri_transpose_tables(BlockTri* bt, const cplx* as_val) {
    if (!bt->has_t) {
        const int64_t N = bt->N, nnz = bt->nnz;
        hipStream_t st = nullptr;
        DevBuf<int> cnt; cnt.alloc((size_t)N);
        LSFC_HIP(hipMemsetAsync(cnt.p, 0, cnt.bytes(), st));
        hipLaunchKernelGGL(k_bt_tcount, dim3(nblk(nnz, 256)), dim3(256), 0, st, nnz, (const int*)bt->col.p, cnt.p);
        LSFC_HIP(hipGetLastError());
        std::vector<int> hcnt((size_t)N);
        LSFC_HIP(hipMemcpyAsync(hcnt.data(), cnt.p, cnt.bytes(), hipMemcpyDeviceToHost, st));
        LSFC_HIP(hipStreamSynchronize(st));
        std::vector<int64_t> hptr((size_t)N + 1, 0);
        for (int64_t c = 0; c < N; ++c) hptr[(size_t)c + 1] = hptr[(size_t)c] + hcnt[(size_t)c];
        LSFC_REQUIRE(hptr[(size_t)N] == nnz, "internal: the transpose of %lld entries has %lld", (long long)nnz, (long long)hptr[(size_t)N]);
        DevBuf<int64_t> tidx; tidx.alloc((size_t)nnz);
        bt->t_rowptr.alloc((size_t)N + 1); bt->t_rlo.alloc((size_t)N); bt->t_rhi.alloc((size_t)N);
        bt->t_col.alloc((size_t)nnz); bt->t_val.alloc((size_t)nnz); bt->t_as.alloc((size_t)nnz);
        LSFC_HIP(hipMemcpyAsync(bt->t_rowptr.p, hptr.data(), hptr.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
        LSFC_HIP(hipMemsetAsync(cnt.p, 0, cnt.bytes(), st));
        // (k_bt_ufill from rowptr[r] on: the whole row)
        hipLaunchKernelGGL(k_bt_ufill, dim3(nblk(N, 256)), dim3(256), 0, st, N, (const int64_t*)bt->rowptr.p, (const int64_t*)bt->rowptr.p, (const int*)bt->col.p,
                           (const int64_t*)bt->t_rowptr.p, cnt.p, bt->t_col.p, tidx.p);
        hipLaunchKernelGGL(k_bt_usort, dim3(nblk(N, 256)), dim3(256), 0, st, N, (const int64_t*)bt->t_rowptr.p, bt->t_col.p, tidx.p, (const cplx*)bt->val.p, bt->t_val.p);
        hipLaunchKernelGGL(k_bt_tsplit, dim3(nblk(N, 256)), dim3(256), 0, st, N, bt->b, (const int64_t*)bt->t_rowptr.p, (const int*)bt->t_col.p,
                           (const int64_t*)tidx.p, as_val, bt->t_rlo.p, bt->t_rhi.p, bt->t_as.p);
        LSFC_HIP(hipGetLastError());
        LSFC_HIP(hipStreamSynchronize(st));
        bt->has_t = true;
    }
    const int64_t bytes = (int64_t)(bt->t_rowptr.bytes() + bt->t_rlo.bytes() + bt->t_rhi.bytes() + bt->t_col.bytes() + bt->t_val.bytes() + bt->t_as.bytes());
    return BlockTriT{bt->t_rowptr.p, bt->t_col.p, bt->t_as.p, bytes};
}

void blocktri_destroy(BlockTri* bt) { delete bt; }
const int* blocktri_col32(const BlockTri* bt) { return bt->col.p; }
int64_t blocktri_nnz(const BlockTri* bt) { return bt->nnz; }

// the stored inverses under their own type: f(S) with S the float pairs or the complex doubles
template <class F> static void with_storage(const BlockTri* bt, F&& f) {
    if (bt->prec == BLOCKTRI_INV_F32) f((const cplx32*)bt->S32.p); else f((const cplx*)bt->S.p);
}

void blocktri_enqueue(const BlockTri* bt, const cplx* w, cplx* x, hipStream_t st, bool transposed) {
    LSFC_REQUIRE(!transposed || bt->has_t, "internal: transposed sweep without its tables");
    const BtApply a = bt->tables(transposed);
    const dim3 wg(AP_ROWS * AP_SLOTS);
    with_storage(bt, [&](auto S) {
        using T = std::remove_const_t<std::remove_pointer_t<decltype(S)>>;
        if (transposed) {
            if (bt->b <= WALK_B) { hipLaunchKernelGGL(k_bt_walk_t<T>, dim3(1), wg, 0, st, a, S, w, x); return; }
            const dim3 g(nblk(bt->b, ST_COLS));
            for (int k = 0; k < (int)bt->K; ++k) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bt_step_t<true, T>), g, wg, 0, st, a, S, k, w, x);
            for (int k = (int)bt->K - 2; k >= 0; --k) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bt_step_t<false, T>), g, wg, 0, st, a, S, k, w, x);
            return;
        }
        if (bt->b <= WALK_B) { hipLaunchKernelGGL(k_bt_walk<T>, dim3(1), wg, 0, st, a, S, w, x); return; }
        const dim3 g(nblk(bt->b, AP_ROWS * BT_LANE_ROWS<T>));
        for (int k = 0; k < (int)bt->K; ++k) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bt_step<true, T>), g, wg, 0, st, a, S, k, w, x);
        for (int k = (int)bt->K - 2; k >= 0; --k) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bt_step<false, T>), g, wg, 0, st, a, S, k, w, x);
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
        using T = std::remove_const_t<std::remove_pointer_t<decltype(S)>>;
        const dim3 pg(nblk(b, BB_ROWS * BT_LANE_ROWS<T>), (unsigned)nranges), pgt(nblk(b, BT_WAVES * wcols), (unsigned)nranges);
        auto step = [&](int k, auto fwd) {
            constexpr bool FWD = decltype(fwd)::value;
            hipLaunchKernelGGL(k_btb_stage<FWD>, dim3(g), dim3(256), 0, st, a, k, R, N, w, (const cplx*)x, t);
            if (transposed)
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_btb_product_t<decltype(rc)::value, T>), pgt, dim3(64 * BT_WAVES), 0, st, S + (int64_t)k * b * b, b, wcols,
                                   range, (const cplx*)t, part);
            else
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_btb_product<decltype(rc)::value, T>), pg, dim3(BB_ROWS * BB_SLOTS), 0, st, S + (int64_t)k * b * b, b, cols,
                                   (const cplx*)t, part);
            hipLaunchKernelGGL(k_btb_fold<FWD>, dim3(g), dim3(256), 0, st, b, k, R, nranges, N, (const cplx*)part, x);
        };
        for (int k = 0; k < (int)bt->K; ++k) step(k, std::true_type{});
        for (int k = (int)bt->K - 2; k >= 0; --k) step(k, std::false_type{});
    }); });
}

BlockTriInfo blocktri_info(const BlockTri* bt) {
    const int64_t bytes = (int64_t)(bt->prec == BLOCKTRI_INV_F32 ? bt->S32.bytes() : bt->S.bytes());
    return BlockTriInfo{bt->K, bt->b, bytes, bt->launches(), bt->factor_us, bt->pivoted ? 1 : 0, bt->min_ratio};
}

void blocktri_get_pivots(const BlockTri* bt, int64_t k, int64_t* host_out) {
    if (!bt->pivoted) { for (int64_t i = 0; i < bt->b; ++i) host_out[i] = i; return; }
    std::vector<int> h((size_t)bt->b);
    LSFC_HIP(hipMemcpy(h.data(), bt->perm.p + k * bt->b, h.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < bt->b; ++i) host_out[i] = h[(size_t)i];
}

int blocktri_precision(const BlockTri* bt) { return bt->prec; }

void blocktri_get_block(const BlockTri* bt, int64_t k, cplx* host_out) {
    const size_t n = (size_t)(bt->b * bt->b);
    if (bt->prec == BLOCKTRI_INV_F32) {                                      // the stored float pairs, widened on the host
        std::vector<cplx32> h(n);
        LSFC_HIP(hipMemcpy(h.data(), bt->S32.p + k * bt->b * bt->b, n * sizeof(cplx32), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) host_out[i] = make_double2((double)h[i].x, (double)h[i].y);
        return;
    }
    LSFC_HIP(hipMemcpy(host_out, bt->S.p + k * bt->b * bt->b, n * sizeof(cplx), hipMemcpyDeviceToHost));
}

__global__ void k_warmup_blocktri(int* p) { if (p) *p = 0; }
void warmup_blocktri() {
    hipLaunchKernelGGL(k_warmup_blocktri, dim3(1), dim3(64), 0, 0, (int*)nullptr);
    LSFC_HIP(hipGetLastError());
}

} // namespace lsfc
