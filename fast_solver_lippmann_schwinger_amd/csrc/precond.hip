// Device-resident apply of the reference's SparsifyingPreconditioner (src/preconditioner.jl:27-58, 132-170):
//
//     v  <-  Msp^{-1} (As v)
//
// As is a sparse matrix (SpMV), Msp^{-1} is applied through the LU factors the caller computed on the host (UMFPACK
// `lu(Msp)` in the reference, src/preconditioner.jl:35): (Rs .* Msp)[p, q] = L U.  The factorisation itself, and the
// assembly of As / Msp, stay on the host and out of scope; what moves to the device is the part that runs once per
// Arnoldi step, so the Krylov vector no longer crosses PCIe twice per step.
//
// Sparse triangular solves by level scheduling: rows are grouped by dependency depth.  The factors of a 2D/3D stencil
// matrix are deep and thin, so four kinds of steps are scheduled at set-up:
//   * a wide or heavy level              one launch over all its rows, 8..64 lanes per row by row length
//   * a run of light, narrow levels      ONE single-workgroup launch that walks them with barriers, 1024 / rows lanes
//                                        per row; consecutive thin levels are fused into groups of <= 16 rows whose
//                                        mutual coupling is a dense 16 x 16 block resolved by one wave in registers
//   * a heavy group                      the same in two launches: one workgroup per row, then the dense block
//   * a long sequence of thin levels     a dense run: coupling stored as a dense R x R block, blocked right-looking
//                                        forward substitution (the trailing separator blocks of the factor)
// The whole sequence SpMV -> L solve -> U solve -> scatter is captured once in a hipGraph on fixed internal buffers
// and replayed per apply.
//
// A second kind of object is factorised on the device (blocktri.hip; lsfc_precond_create_blocktri / _from_plan at the end
// of this file): its apply is the same SpMV followed by the block-tridiagonal sweeps, captured and replayed the same way.
// Such an object also takes GROUPS of up to 8 vectors (precond_apply_batch_dev, lsfc_precond_apply_batch): one SpMV launch
// and one sweep per group, As and every S_k^{-1} read once per group; one captured graph per group size.
// Under lsfc_precond_set_op(T | H) it applies the transpose As^T Msp^{-T} (the transposed sweeps of blocktri.hip first, then
// the SpMV with As^T) or the adjoint (the same between two conjugating copies), single and in groups, from graphs of their own.
#include "common.hpp"
#include "pruned.hpp"
#include "plan.hpp"
#include "blocktri.hpp"
#include <algorithm>
#include <complex>
#include <cstring>
#include <memory>
#include <vector>

namespace lsfc {

// ---- kernels -------------------------------------------------------------------------------------------------------

// y[k] = scale[row] * sum_j A[row, j] x[j],  row = gather[k]   (CSR, LPR lanes per row)
template <int LPR>
__global__ void k_spmv_gather(const int64_t* __restrict__ rowptr, const int* __restrict__ col, const cplx* __restrict__ val,
                              const int* __restrict__ gather, const double* __restrict__ scale, const cplx* __restrict__ x,
                              cplx* __restrict__ y, int nrows) {
    const int g = (int)((blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / LPR), lane = threadIdx.x % LPR;
    if (g >= nrows) return;                       // (whole LPR-groups leave together: blockDim is a multiple of LPR)
    const int row = gather ? gather[g] : g;
    double sx = 0.0, sy = 0.0;
    for (int64_t e = rowptr[row] + lane; e < rowptr[row + 1]; e += LPR) {
        const cplx a = val[e], b = x[col[e]];
        sx += a.x * b.x - a.y * b.y; sy += a.x * b.y + a.y * b.x;
    }
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) { sx += __shfl_xor(sx, o, LPR); sy += __shfl_xor(sy, o, LPR); }
    if (lane == 0) { const double s = scale ? scale[row] : 1.0; y[g] = make_double2(s * sx, s * sy); }
}

// The same for R vectors (member-major, member r at x + r n and y + r n; no gather, no scale): the row of the matrix is
// read once and applied to every member.  Multiply-adds spelled out, one set of sums per member: the bits of a member's
// result do not depend on R or on its place in the group.
template <int R>
__global__ void k_spmv_batch(const int64_t* __restrict__ rowptr, const int* __restrict__ col, const cplx* __restrict__ val,
                             const cplx* __restrict__ x, cplx* __restrict__ y, int nrows) {
    constexpr int LPR = 8;
    const int row = (int)((blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / LPR), lane = threadIdx.x % LPR;
    if (row >= nrows) return;                     // (whole LPR-groups leave together: blockDim is a multiple of LPR)
    double sx[R], sy[R];
#pragma unroll
    for (int r = 0; r < R; ++r) { sx[r] = 0.0; sy[r] = 0.0; }
    for (int64_t e = rowptr[row] + lane; e < rowptr[row + 1]; e += LPR) {
        const cplx a = val[e];
        const int c = col[e];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const cplx b = x[(int64_t)r * nrows + c];
            sx[r] = fma(a.x, b.x, sx[r]); sx[r] = fma(-a.y, b.y, sx[r]);
            sy[r] = fma(a.x, b.y, sy[r]); sy[r] = fma(a.y, b.x, sy[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int o = LPR / 2; o > 0; o >>= 1) { sx[r] += __shfl_xor(sx[r], o, LPR); sy[r] += __shfl_xor(sy[r], o, LPR); }
        if (lane == 0) y[(int64_t)r * nrows + row] = make_double2(sx[r], sy[r]);
    }
}

// the vectors of a group, wherever they live, into / out of the member-major work buffer (TO_WORK: work <- v, else v <- work)
// CONJ: the copy conjugates (the adjoint apply is conj . transposed apply . conj, with both conjugations in these copies)
struct GroupPtrs { cplx* v[LSFC_MAX_BATCH]; };
template <bool TO_WORK, bool CONJ = false>
__global__ void k_group_copy(GroupPtrs g, cplx* __restrict__ work, int64_t n) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    cplx* v = g.v[blockIdx.y];
    cplx s = TO_WORK ? v[i] : work[(int64_t)blockIdx.y * n + i];
    if (CONJ) s.y = -s.y;
    if (TO_WORK) work[(int64_t)blockIdx.y * n + i] = s; else v[i] = s;
}

// one row of a triangular solve, LANES lanes: x[row] = (b[row] - sum_{j != row} a_j x[col_j]) * inv_diag
// (rows are stored in level order: entry k of the sorted arrays is original row rowid[k]; off-diagonal entries only)
template <int LANES>
__device__ __forceinline__ void trsv_row(int k, int lane, const int64_t* __restrict__ rowptr, const int* __restrict__ col,
                                         const cplx* __restrict__ val, const int* __restrict__ rowid, const cplx* __restrict__ invd,
                                         const cplx* __restrict__ b, cplx* x) {
    double sx = 0.0, sy = 0.0;
    for (int64_t e = rowptr[k] + lane; e < rowptr[k + 1]; e += LANES) {
        const cplx a = val[e], v = x[col[e]];
        sx += a.x * v.x - a.y * v.y; sy += a.x * v.y + a.y * v.x;
    }
#pragma unroll
    for (int o = LANES / 2; o > 0; o >>= 1) { sx += __shfl_xor(sx, o, LANES); sy += __shfl_xor(sy, o, LANES); }
    if (lane == 0) {
        const int row = rowid[k];
        const cplx r = make_double2(b[row].x - sx, b[row].y - sy), d = invd[k];
        x[row] = make_double2(r.x * d.x - r.y * d.y, r.x * d.y + r.y * d.x);
    }
}

// one level as its own launch over many workgroups: rows [first, first + nrows) of the sorted order, LPR lanes per row
// (8 for the short rows of the early levels, a whole wave for the long rows of the fill)
template <int LPR>
__global__ void k_trsv_level(int first, int nrows, const int64_t* __restrict__ rowptr, const int* __restrict__ col, const cplx* __restrict__ val,
                             const int* __restrict__ rowid, const cplx* __restrict__ invd, const cplx* __restrict__ b, cplx* x) {
    const int g = (int)((blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / LPR), lane = threadIdx.x % LPR;
    if (g >= nrows) return;
    trsv_row<LPR>(first + g, lane, rowptr, col, val, rowid, invd, b, x);
}

// a run of narrow levels in ONE workgroup of 1024 threads, a barrier between steps.  The tail of a sparse LU factor
// is deep and thin -- at 2D 257 x 257 a third of the fill sits in 1391 levels of ONE row with ~740 entries each (the
// dense trailing separator blocks) -- so
//  * the lanes are dealt out per step: 1024 / (rows rounded up to a power of two) lanes per row, all 1024 on a single
//    row; sums are folded by wave shuffles and, beyond one wave per row, through LDS;
//  * consecutive thin levels are fused into GROUPS of at most 16 rows: the entries that couple rows of the same group
//    are taken out of the CSR rows into a dense 16 x 16 block at set-up, every row of the group sums its remaining
//    (external) entries at the same time, and one wave then resolves the little dense triangle in registers
//    (16 shuffle steps, no memory latency).  One barrier-bound step thus retires up to 16 dependency levels.
// A group with dense offset -1 is a single level (independent rows).
static constexpr int GROUP_ROWS = 16;

// shared by the walking kernel and the heavy-group kernel: lanes i < nrows of ONE wave hold acc_i = b_i - (external sum);
// forward substitution through the dense block, x_i written by lane i
__device__ __forceinline__ void dense_resolve(int i, int nrows, int first, int dofs, double ax, double ay, const cplx* __restrict__ dense,
                                              const int* __restrict__ rowid, const cplx* __restrict__ invd, cplx* x) {
    const bool mine = i < nrows;
    const cplx di = mine ? invd[first + i] : make_double2(0.0, 0.0);
    cplx drow[GROUP_ROWS];
#pragma unroll
    for (int j = 0; j < GROUP_ROWS; ++j) drow[j] = (mine && j < i) ? dense[(int64_t)dofs + i * GROUP_ROWS + j] : make_double2(0.0, 0.0);
    double myx = 0.0, myy = 0.0;
#pragma unroll
    for (int j = 0; j < GROUP_ROWS; ++j) {
        if (j < nrows) {                                       // uniform
            const double tx = ax * di.x - ay * di.y, ty = ax * di.y + ay * di.x;      // x_j on lane j
            const double xjx = __shfl(tx, j, 64), xjy = __shfl(ty, j, 64);
            if (i == j) { myx = xjx; myy = xjy; }
            ax -= drow[j].x * xjx - drow[j].y * xjy; ay -= drow[j].x * xjy + drow[j].y * xjx;
        }
    }
    if (mine) x[rowid[first + i]] = make_double2(myx, myy);
}


__global__ __launch_bounds__(1024)
void k_trsv_chain(int g0, int g1, const int* __restrict__ grpptr, const int* __restrict__ grpcnt, const int* __restrict__ grpdense,
                  const cplx* __restrict__ dense,
                  const int64_t* __restrict__ rowptr, const int* __restrict__ col, const cplx* __restrict__ val,
                  const int* __restrict__ rowid, const cplx* __restrict__ invd, const cplx* __restrict__ b, cplx* x) {
    __shared__ double psx[16], psy[16], rx[GROUP_ROWS], ry[GROUP_ROWS];
    const int tid = threadIdx.x, wave = tid >> 6;
    for (int gi = g0; gi < g1; ++gi) {
        const int first = grpptr[gi], nrows = grpcnt[gi], dofs = grpdense[gi];     // uniform over the workgroup
        int p2 = 1; while (p2 < nrows) p2 <<= 1;
        const int lanes = 1024 / p2;                                       // 8 ... 1024, a power of two
        const int g = tid / lanes, lane = tid % lanes;
        const bool active = g < nrows;
        const int k = first + (active ? g : 0);
        double sx = 0.0, sy = 0.0;
        if (active) {
            const int64_t e1 = rowptr[k + 1];
#pragma unroll 4
            for (int64_t e = rowptr[k] + lane; e < e1; e += lanes) {
                const cplx a = val[e], v = x[col[e]];
                sx += a.x * v.x - a.y * v.y; sy += a.x * v.y + a.y * v.x;
            }
        }
        const int wl = lanes < 64 ? lanes : 64;                            // lanes of this row inside one wave
        for (int o = wl >> 1; o > 0; o >>= 1) { sx += __shfl_xor(sx, o, 64); sy += __shfl_xor(sy, o, 64); }
        if (lanes > 64) {                                                  // several waves per row: fold through LDS
            if ((tid & 63) == 0) { psx[wave] = sx; psy[wave] = sy; }
            __syncthreads();
            if (lane == 0) {
                const int nw = lanes >> 6;
                sx = 0.0; sy = 0.0;
                for (int w = 0; w < nw; ++w) { sx += psx[wave + w]; sy += psy[wave + w]; }
            }
        }
        if (dofs < 0) {                                                    // independent rows
            if (active && lane == 0) {
                const int row = rowid[k];
                const cplx r = make_double2(b[row].x - sx, b[row].y - sy), d = invd[k];
                x[row] = make_double2(r.x * d.x - r.y * d.y, r.x * d.y + r.y * d.x);
            }
        } else {                                                           // rows coupled through the dense block
            if (active && lane == 0) { const int row = rowid[k]; rx[g] = b[row].x - sx; ry[g] = b[row].y - sy; }
            __syncthreads();
            if (wave == 0) dense_resolve(tid, nrows, first, dofs, tid < nrows ? rx[tid] : 0.0, tid < nrows ? ry[tid] : 0.0, dense, rowid, invd, x);
        }
        __syncthreads();                          // this step's rows are visible to the next step (same workgroup)
    }
}
// (tried: loading the descriptor and first matrix entry of the next step while the current one is reduced -- slower:
// the walk is bound by the barrier / reduction chain, not by those loads)

// A HEAVY group (<= 16 coupled rows with more entries than one CU should stream) as two launches:
//   k_trsv_group_ext   one 512-thread workgroup per row sums the row's external entries (many CUs, whole rows in flight)
//   k_trsv_group_dense one wave resolves the dense coupling block from those sums and writes x
__global__ __launch_bounds__(512)
void k_trsv_group_ext(int first, const int64_t* __restrict__ rowptr, const int* __restrict__ col, const cplx* __restrict__ val,
                      const int* __restrict__ rowid, const cplx* __restrict__ b, const cplx* __restrict__ x, cplx* __restrict__ gacc) {
    __shared__ double psx[8], psy[8];
    const int k = first + blockIdx.x, tid = threadIdx.x;
    double sx = 0.0, sy = 0.0;
    const int64_t e1 = rowptr[k + 1];
#pragma unroll 4
    for (int64_t e = rowptr[k] + tid; e < e1; e += 512) {
        const cplx a = val[e], v = x[col[e]];
        sx += a.x * v.x - a.y * v.y; sy += a.x * v.y + a.y * v.x;
    }
    for (int o = 32; o > 0; o >>= 1) { sx += __shfl_xor(sx, o, 64); sy += __shfl_xor(sy, o, 64); }
    if ((tid & 63) == 0) { psx[tid >> 6] = sx; psy[tid >> 6] = sy; }
    __syncthreads();
    if (tid == 0) {
        sx = 0.0; sy = 0.0;
        for (int w = 0; w < 8; ++w) { sx += psx[w]; sy += psy[w]; }
        const int row = rowid[k];
        gacc[blockIdx.x] = make_double2(b[row].x - sx, b[row].y - sy);
    }
}

__global__ __launch_bounds__(64)
void k_trsv_group_dense(int first, int nrows, int dofs, const cplx* __restrict__ dense, const int* __restrict__ rowid,
                        const cplx* __restrict__ invd, const cplx* __restrict__ gacc, cplx* x) {
    const int i = threadIdx.x;
    const cplx a = i < nrows ? gacc[i] : make_double2(0.0, 0.0);
    dense_resolve(i, nrows, first, dofs, a.x, a.y, dense, rowid, invd, x);
}

// A dense RUN: a long sequence of consecutive thin levels (the trailing separator block of a sparse LU factor is a
// chain of one-row levels, each row coupled to almost all rows before it).  Its R rows are solved as a dense
// lower-triangular system in blocks of 64, right-looking:
//   k_run_ext     acc_i = b_i - (entries outside the run), one workgroup per row                       1 launch
//   k_run_diag    one wave solves the 64 x 64 diagonal block J from acc (block staged in LDS)          R / 64 launches
//   k_run_update  acc_i -= D[i, block J] x_J for the rows below, one wave per row, many CUs            R / 64 - 1 launches
// The coupling D is stored dense (R x R, row-major), taken out of the CSR rows at set-up.
static constexpr int RUN_BLOCK = 64;

__global__ __launch_bounds__(256)
void k_run_ext(int first, const int64_t* __restrict__ rowptr, const int* __restrict__ col, const cplx* __restrict__ val,
               const int* __restrict__ rowid, const cplx* __restrict__ b, const cplx* __restrict__ x, cplx* __restrict__ racc) {
    __shared__ double psx[4], psy[4];
    const int k = first + blockIdx.x, tid = threadIdx.x;
    double sx = 0.0, sy = 0.0;
    const int64_t e1 = rowptr[k + 1];
#pragma unroll 4
    for (int64_t e = rowptr[k] + tid; e < e1; e += 256) {
        const cplx a = val[e], v = x[col[e]];
        sx += a.x * v.x - a.y * v.y; sy += a.x * v.y + a.y * v.x;
    }
    for (int o = 32; o > 0; o >>= 1) { sx += __shfl_xor(sx, o, 64); sy += __shfl_xor(sy, o, 64); }
    if ((tid & 63) == 0) { psx[tid >> 6] = sx; psy[tid >> 6] = sy; }
    __syncthreads();
    if (tid == 0) {
        const int row = rowid[k];
        racc[blockIdx.x] = make_double2(b[row].x - (psx[0] + psx[1] + psx[2] + psx[3]), b[row].y - (psy[0] + psy[1] + psy[2] + psy[3]));
    }
}

__global__ __launch_bounds__(64)
void k_run_diag(int first, int R, int J, const cplx* __restrict__ D, const int* __restrict__ rowid, const cplx* __restrict__ invd,
                const cplx* __restrict__ racc, cplx* __restrict__ rx, cplx* x) {
    __shared__ cplx blk[RUN_BLOCK][RUN_BLOCK + 1];
    const int lane = threadIdx.x, r0 = J * RUN_BLOCK;
    const int nb = R - r0 < RUN_BLOCK ? R - r0 : RUN_BLOCK;
    for (int r = 0; r < nb; ++r) if (lane < nb) blk[r][lane] = D[(int64_t)(r0 + r) * R + r0 + lane];   // row r, coalesced
    __syncthreads();
    const bool mine = lane < nb;
    cplx acc = mine ? racc[r0 + lane] : make_double2(0.0, 0.0);
    const cplx di = mine ? invd[first + r0 + lane] : make_double2(0.0, 0.0);
    double myx = 0.0, myy = 0.0;
    for (int j = 0; j < nb; ++j) {
        const double tx = acc.x * di.x - acc.y * di.y, ty = acc.x * di.y + acc.y * di.x;                  // x_j on lane j
        const double xjx = __shfl(tx, j, 64), xjy = __shfl(ty, j, 64);
        if (lane == j) { myx = xjx; myy = xjy; }
        if (mine && lane > j) { const cplx d = blk[lane][j]; acc.x -= d.x * xjx - d.y * xjy; acc.y -= d.x * xjy + d.y * xjx; }
    }
    if (mine) { const cplx v = make_double2(myx, myy); rx[r0 + lane] = v; x[rowid[first + r0 + lane]] = v; }
}

__global__ __launch_bounds__(256)
void k_run_update(int R, int J, const cplx* __restrict__ D, const cplx* __restrict__ rx, cplx* __restrict__ racc) {
    const int lane = threadIdx.x & 63, r0 = J * RUN_BLOCK;
    const int i = r0 + RUN_BLOCK + (int)blockIdx.x * 4 + (threadIdx.x >> 6);          // a wave per row below block J
    if (i >= R) return;                                                               // (whole waves leave together)
    const cplx d = D[(int64_t)i * R + r0 + lane], v = rx[r0 + lane];                  // block J is a full block here
    double sx = d.x * v.x - d.y * v.y, sy = d.x * v.y + d.y * v.x;
    for (int o = 32; o > 0; o >>= 1) { sx += __shfl_xor(sx, o, 64); sy += __shfl_xor(sy, o, 64); }
    if (lane == 0) { cplx a = racc[i]; a.x -= sx; a.y -= sy; racc[i] = a; }
}

__global__ void k_scatter(const cplx* __restrict__ w, const int* __restrict__ dst, cplx* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[dst[i]] = w[i];
}

// ---- host side -------------------------------------------------------------------------------------------------------

struct TriFactor {                 // one triangular factor, rows in level order
    DevBuf<int64_t> rowptr; DevBuf<int> col; DevBuf<cplx> val; DevBuf<int> rowid; DevBuf<cplx> invd; DevBuf<int> lvlptr;
    std::vector<int> h_lvlptr;     // host copy of the level boundaries
    int nlevels = 0;
    // launch schedule: kind 0 one level [l0, l0 + 1) as its own launch (lpr lanes per row); 1 a run of groups [l0, l1) walked by
    // one workgroup; 2 the heavy group l0 as two launches; 3 the dense run l0
    struct Seg { int kind; int l0, l1; int lpr; };
    std::vector<Seg> segs;
    DevBuf<int> grpptr, grpcnt, grpdense; DevBuf<cplx> dense;            // groups of the chain segments
    std::vector<int> h_grpptr, h_grpcnt, h_grpdense;
    DevBuf<cplx> gacc;                                                   // b - external sums of a heavy group
    struct Run { int first, R; int64_t dofs; };                         // dense runs: first sorted row, rows, offset of the R x R block
    std::vector<Run> runs;
    DevBuf<cplx> rdense, racc, rx;
    int ngroups = 0;
    int64_t sched[10] = {};        // what the schedule reached (lsfc_precond_schedule, include/lsfc.h)
};

static int narrow_rows() {               // levels with at most this many rows (default 32: 42 -> 37 ms at N = 263 169 against
                                         // 128; LSFC_PRECOND_NARROW, 8..128) ...
    static const int v = [] { const char* e = getenv("LSFC_PRECOND_NARROW"); int n = e ? atoi(e) : 32; return n < 8 ? 8 : (n > 128 ? 128 : n); }();
    return v;
}
#define NARROW narrow_rows()
static constexpr int64_t CHAIN_NNZ = 8192; // ... and at most this many entries are walked inside a single workgroup
static constexpr int RUN_THIN = 4;        // dense runs: consecutive levels of at most this many rows ...
static constexpr int RUN_MIN = 96;        // ... totalling at least this many rows, cut into pieces of at most
static constexpr int RUN_MAX = 1024;      // this many rows (R x R dense block: 16 MB)

static void build_factor(TriFactor& F, int64_t N, const int64_t* rowptr, const int64_t* col, const double* val, bool lower) {
    // levels: depth of each row in the dependency graph of the triangular solve
    std::vector<int> level((size_t)N, 0);
    std::vector<std::complex<double>> diag((size_t)N, std::complex<double>(0, 0));
    int nlev = 0;
    auto scan_row = [&](int64_t r) {
        int lv = 0; bool have_diag = false;
        for (int64_t e = rowptr[r]; e < rowptr[r + 1]; ++e) {
            const int64_t c = col[e];
            LSFC_REQUIRE(c >= 0 && c < N, "preconditioner factor: column index out of range");
            if (c == r) { diag[(size_t)r] = std::complex<double>(val[2 * e], val[2 * e + 1]); have_diag = true; continue; }
            LSFC_REQUIRE(lower ? c < r : c > r, "preconditioner factor: %s factor has an entry on the wrong side of the diagonal (row %lld, col %lld)",
                         lower ? "L" : "U", (long long)r, (long long)c);
            lv = std::max(lv, level[(size_t)c] + 1);
        }
        LSFC_REQUIRE(have_diag && diag[(size_t)r] != std::complex<double>(0, 0), "preconditioner factor: zero or missing diagonal in row %lld", (long long)r);
        level[(size_t)r] = lv; nlev = std::max(nlev, lv + 1);
    };
    if (lower) for (int64_t r = 0; r < N; ++r) scan_row(r); else for (int64_t r = N - 1; r >= 0; --r) scan_row(r);
    // counting sort of the rows by level
    std::vector<int> lvlptr((size_t)nlev + 1, 0);
    for (int64_t r = 0; r < N; ++r) ++lvlptr[(size_t)level[(size_t)r] + 1];
    for (int l = 0; l < nlev; ++l) lvlptr[(size_t)l + 1] += lvlptr[(size_t)l];
    std::vector<int> order((size_t)N), fill(lvlptr.begin(), lvlptr.end() - 1);
    for (int64_t r = 0; r < N; ++r) order[(size_t)fill[(size_t)level[(size_t)r]]++] = (int)r;
    // schedule: a wide level is one launch; a run of consecutive narrow levels is one single-workgroup launch that walks
    // GROUPS: consecutive thin levels with at most GROUP_ROWS rows together, coupled through a dense block
    std::vector<int> grpptr, grpcnt, grpdense;      // group -> first sorted row, rows, dense offset (-1: a single level)
    std::vector<int> group_of((size_t)N, -1);       // sorted row -> group, for the rows of multi-level groups only
    int64_t ndense = 0;
    // a level is walked inside the single-workgroup chain only if it is narrow AND light (one CU streams it); a level
    // with many rows or many entries gets its own launch over many CUs, a wave per row when the rows are long
    std::vector<int64_t> lvlnnz((size_t)nlev, 0);
    for (int64_t r = 0; r < N; ++r) lvlnnz[(size_t)level[(size_t)r]] += rowptr[r + 1] - rowptr[r] - 1;
    // dense runs: long sequences of consecutive thin levels (trailing separator blocks), cut into pieces of <= RUN_MAX rows
    std::vector<int> run_of_level((size_t)nlev, -1), run_of((size_t)N, -1);
    int64_t nrdense = 0;
    for (int l = 0; l < nlev;) {
        int e = l, rows = 0;
        while (e < nlev && lvlptr[(size_t)e + 1] - lvlptr[(size_t)e] <= RUN_THIN) { rows += lvlptr[(size_t)e + 1] - lvlptr[(size_t)e]; ++e; }
        if (rows < RUN_MIN) { l = e > l ? e : l + 1; continue; }
        while (l < e) {                             // pieces end at level boundaries
            int pe = l, prow = 0;
            while (pe < e && prow + (lvlptr[(size_t)pe + 1] - lvlptr[(size_t)pe]) <= RUN_MAX) { prow += lvlptr[(size_t)pe + 1] - lvlptr[(size_t)pe]; ++pe; }
            const int ri = (int)F.runs.size();
            F.runs.push_back({lvlptr[(size_t)l], prow, nrdense});
            nrdense += (int64_t)prow * prow;
            for (int q = l; q < pe; ++q) run_of_level[(size_t)q] = ri;
            for (int k = lvlptr[(size_t)l]; k < lvlptr[(size_t)pe]; ++k) run_of[(size_t)k] = ri;
            l = pe;
        }
    }
    auto chainable = [&](int l) { return run_of_level[(size_t)l] < 0 && lvlptr[(size_t)l + 1] - lvlptr[(size_t)l] <= NARROW && lvlnnz[(size_t)l] <= CHAIN_NNZ; };
    for (int l = 0; l < nlev;) {
        const int rows = lvlptr[(size_t)l + 1] - lvlptr[(size_t)l];
        if (run_of_level[(size_t)l] >= 0) {         // a dense run: its own sequence of launches
            const int ri = run_of_level[(size_t)l];
            F.segs.push_back({3, ri, ri + 1, 0});
            while (l < nlev && run_of_level[(size_t)l] == ri) ++l;
            continue;
        }
        if (!chainable(l)) {                        // lanes per row ~ entries per row
            const int64_t avg = lvlnnz[(size_t)l] / (rows > 0 ? rows : 1);
            F.segs.push_back({0, l, l + 1, avg >= 48 ? 64 : (avg >= 24 ? 32 : (avg >= 12 ? 16 : 8))}); ++l; continue;
        }
        int gfirst = (int)grpptr.size();
        while (l < nlev && chainable(l)) {
            int e = l + 1, tot = lvlptr[(size_t)l + 1] - lvlptr[(size_t)l];
            int64_t gnnz = lvlnnz[(size_t)l];
            while (e < nlev && chainable(e) && tot + (lvlptr[(size_t)e + 1] - lvlptr[(size_t)e]) <= GROUP_ROWS) {
                tot += lvlptr[(size_t)e + 1] - lvlptr[(size_t)e]; gnnz += lvlnnz[(size_t)e]; ++e;
            }
            grpptr.push_back(lvlptr[(size_t)l]); grpcnt.push_back(tot);
            if (e > l + 1) {                        // several levels: rows coupled through a dense block
                for (int k = lvlptr[(size_t)l]; k < lvlptr[(size_t)e]; ++k) group_of[(size_t)k] = (int)grpdense.size();
                grpdense.push_back((int)ndense); ndense += GROUP_ROWS * GROUP_ROWS;
                if (gnnz > CHAIN_NNZ) {             // too much for one CU: its own pair of launches, the walk resumes after it
                    const int gi = (int)grpptr.size() - 1;
                    if (gi > gfirst) F.segs.push_back({1, gfirst, gi, 0});
                    F.segs.push_back({2, gi, gi + 1, 0});
                    gfirst = gi + 1;
                }
            } else grpdense.push_back(-1);
            l = e;
        }
        if ((int)grpptr.size() > gfirst) F.segs.push_back({1, gfirst, (int)grpptr.size(), 0});
    }
    LSFC_REQUIRE(ndense < ((int64_t)1 << 31), "preconditioner factor: too many dense blocks");
    // sorted CSR without the diagonal; entries coupling two rows of the same group go to that group's dense block
    std::vector<int> sorted_of((size_t)N);
    for (int64_t k = 0; k < N; ++k) sorted_of[(size_t)order[(size_t)k]] = (int)k;
    std::vector<cplx> dense((size_t)ndense, make_double2(0.0, 0.0)), rdense((size_t)nrdense, make_double2(0.0, 0.0));
    std::vector<int64_t> rp((size_t)N + 1, 0);
    std::vector<int> cc; std::vector<cplx> vv; std::vector<cplx> invd((size_t)N);
    cc.reserve((size_t)(rowptr[N])); vv.reserve((size_t)(rowptr[N]));
    for (int64_t k = 0; k < N; ++k) {
        const int64_t r = order[(size_t)k];
        const int grp = group_of[(size_t)k];
        for (int64_t e = rowptr[r]; e < rowptr[r + 1]; ++e) {
            if (col[e] == r) continue;
            const int kc = sorted_of[(size_t)col[e]];
            if (run_of[(size_t)k] >= 0 && run_of[(size_t)kc] == run_of[(size_t)k]) {
                const TriFactor::Run& rn = F.runs[(size_t)run_of[(size_t)k]];
                const int i = (int)k - rn.first, j = kc - rn.first;                             // local indices, j < i
                LSFC_REQUIRE(j >= 0 && j < i && i < rn.R, "internal: run block index (%d, %d)", i, j);
                rdense[(size_t)(rn.dofs + (int64_t)i * rn.R + j)] = make_double2(val[2 * e], val[2 * e + 1]);
                continue;
            }
            if (grp >= 0 && group_of[(size_t)kc] == grp) {
                const int i = (int)k - grpptr[(size_t)grp], j = kc - grpptr[(size_t)grp];       // local indices, j < i
                LSFC_REQUIRE(j >= 0 && j < i && i < GROUP_ROWS, "internal: dense block index (%d, %d)", i, j);
                dense[(size_t)grpdense[(size_t)grp] + (size_t)i * GROUP_ROWS + (size_t)j] = make_double2(val[2 * e], val[2 * e + 1]);
                continue;
            }
            cc.push_back((int)col[e]); vv.push_back(make_double2(val[2 * e], val[2 * e + 1]));
        }
        rp[(size_t)k + 1] = (int64_t)cc.size();
        const std::complex<double> id = 1.0 / diag[(size_t)r];
        invd[(size_t)k] = make_double2(id.real(), id.imag());
    }
    auto up = [](auto& dev, const auto& host) {
        dev.alloc(host.size());
        if (!host.empty()) LSFC_HIP(hipMemcpy(dev.p, host.data(), host.size() * sizeof(host[0]), hipMemcpyHostToDevice));
    };
    up(F.rowptr, rp); up(F.col, cc); up(F.val, vv); up(F.rowid, order); up(F.invd, invd); up(F.lvlptr, lvlptr);
    up(F.grpptr, grpptr); up(F.grpcnt, grpcnt); up(F.grpdense, grpdense); up(F.dense, dense);
    F.h_grpptr = grpptr; F.h_grpcnt = grpcnt; F.h_grpdense = grpdense;
    F.gacc.alloc(GROUP_ROWS);
    up(F.rdense, rdense); F.racc.alloc(RUN_MAX); F.rx.alloc(RUN_MAX);
    F.h_lvlptr = lvlptr; F.nlevels = nlev; F.ngroups = (int)grpdense.size();
    // schedule counts: kind-0 levels by lanes per row, chain segments and their multi-level groups, heavy groups, run pieces
    for (const auto& sg : F.segs) {
        if (sg.kind == 0) ++F.sched[sg.lpr == 64 ? 3 : (sg.lpr == 32 ? 2 : (sg.lpr == 16 ? 1 : 0))];
        else if (sg.kind == 1) { ++F.sched[4]; for (int gi = sg.l0; gi < sg.l1; ++gi) F.sched[5] += grpdense[(size_t)gi] >= 0; }
        else if (sg.kind == 2) ++F.sched[6];
        else {
            const int R = F.runs[(size_t)sg.l0].R;
            F.sched[8] = F.sched[7] ? std::max<int64_t>(F.sched[8], R) : R;
            F.sched[9] = F.sched[7] ? std::min<int64_t>(F.sched[9], R) : R;
            ++F.sched[7];
        }
    }
}

static void launch_factor(const TriFactor& F, const cplx* b, cplx* x, hipStream_t st) {
    for (const auto& s : F.segs) {
        if (s.kind == 1) {
            hipLaunchKernelGGL(k_trsv_chain, dim3(1), dim3(1024), 0, st, s.l0, s.l1, F.grpptr.p, F.grpcnt.p, F.grpdense.p, F.dense.p,
                               F.rowptr.p, F.col.p, F.val.p, F.rowid.p, F.invd.p, b, x);
        } else if (s.kind == 3) {
            const TriFactor::Run& r = F.runs[(size_t)s.l0];
            const cplx* D = F.rdense.p + r.dofs;
            hipLaunchKernelGGL(k_run_ext, dim3((unsigned)r.R), dim3(256), 0, st, r.first, F.rowptr.p, F.col.p, F.val.p, F.rowid.p, b, x, F.racc.p);
            for (int J = 0; J * RUN_BLOCK < r.R; ++J) {
                hipLaunchKernelGGL(k_run_diag, dim3(1), dim3(64), 0, st, r.first, r.R, J, D, F.rowid.p, F.invd.p, F.racc.p, F.rx.p, x);
                const int rem = r.R - (J + 1) * RUN_BLOCK;
                if (rem > 0) hipLaunchKernelGGL(k_run_update, dim3((unsigned)((rem + 3) / 4)), dim3(256), 0, st, r.R, J, D, F.rx.p, F.racc.p);
            }
        } else if (s.kind == 2) {
            const int first = F.h_grpptr[(size_t)s.l0], nrows = F.h_grpcnt[(size_t)s.l0], dofs = F.h_grpdense[(size_t)s.l0];
            hipLaunchKernelGGL(k_trsv_group_ext, dim3((unsigned)nrows), dim3(512), 0, st, first, F.rowptr.p, F.col.p, F.val.p, F.rowid.p, b, x, F.gacc.p);
            hipLaunchKernelGGL(k_trsv_group_dense, dim3(1), dim3(64), 0, st, first, nrows, dofs, F.dense.p, F.rowid.p, F.invd.p, F.gacc.p, x);
        } else {
            const int first = F.h_lvlptr[(size_t)s.l0], nrows = F.h_lvlptr[(size_t)s.l0 + 1] - first;
#define LSFC_LEVEL(LPR) hipLaunchKernelGGL(k_trsv_level<LPR>, dim3((unsigned)(((int64_t)nrows * LPR + 255) / 256)), dim3(256), 0, st, first, nrows, \
                                          F.rowptr.p, F.col.p, F.val.p, F.rowid.p, F.invd.p, b, x)
            switch (s.lpr) { case 64: LSFC_LEVEL(64); break; case 32: LSFC_LEVEL(32); break; case 16: LSFC_LEVEL(16); break; default: LSFC_LEVEL(8); }
#undef LSFC_LEVEL
        }
    }
}

// LSFC_PRECOND_GRAPH=0 (developer switch): plain stream launches instead of the captured graphs
static bool graphs_enabled() {
    static const bool v = !(getenv("LSFC_PRECOND_GRAPH") && getenv("LSFC_PRECOND_GRAPH")[0] == '0');
    return v;
}

// A fixed sequence of launches on internal buffers only, captured once in a hipGraph and replayed from then on.
struct CapturedSeq {
    hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
    CapturedSeq() = default;
    CapturedSeq(const CapturedSeq&) = delete; CapturedSeq& operator=(const CapturedSeq&) = delete;
    ~CapturedSeq() {
        if (exec) (void)hipGraphExecDestroy(exec);
        if (graph) (void)hipGraphDestroy(graph);
    }
    // what enqueue(stream) queues, on `st`; `group`: the group size that the sequence is for, 0 for the single apply
    template <class F> void replay(hipStream_t st, int group, F&& enqueue) {
        if (!graphs_enabled()) { enqueue(st); LSFC_HIP(hipGetLastError()); return; }
        if (!exec) {
            hipStream_t cs; LSFC_HIP(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
            hipError_t e = hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal);
            if (e == hipSuccess) {
                enqueue(cs);
                e = hipStreamEndCapture(cs, &graph);
            }
            if (e == hipSuccess) e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
            (void)hipStreamDestroy(cs);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                if (group) fail(LSFC_EHIP, "preconditioner: graph capture of a group of %d failed: %s", group, hipGetErrorString(e));
                fail(LSFC_EHIP, "preconditioner: graph capture failed: %s", hipGetErrorString(e));
            }
        }
        LSFC_HIP(hipGraphLaunch(exec, st));
    }
};

} // namespace lsfc

struct lsfc_precond {
    int device = 0;
    int64_t N = 0;
    hipStream_t stream = nullptr;
    lsfc::DevBuf<int64_t> a_rowptr; lsfc::DevBuf<int> a_col; lsfc::DevBuf<lsfc::cplx> a_val;     // As, CSR
    lsfc::DevBuf<int> rgather, cscatter; lsfc::DevBuf<double> rscale;
    lsfc::TriFactor L, U;
    lsfc::BlockTri* bt = nullptr;      // block-tridiagonal factorisation (blocktri.hip) instead of L, U
    lsfc::DevBuf<lsfc::cplx> vin, y0, z, w, vout;
    lsfc::DevBuf<lsfc::cplx> hstage;   // host vectors of lsfc_precond_apply and _apply_batch pass through here, grown on demand
    lsfc::CapturedSeq seq;             // SpMV and solves of one apply
    int launches = 0;
    // groups of right-hand sides (block-tridiagonal objects): member-major work buffers for bcap members, one graph per group size
    lsfc::DevBuf<lsfc::cplx> bvin, by0, bvout;
    int bcap = 0;
    std::unique_ptr<lsfc::CapturedSeq[]> bseq;      // indexed by group size
    int64_t bsweeps = 0, bvectors = 0, blargest = 0, bwork_bytes = 0;
    // what the applies compute (lsfc_precond_set_op): Msp^{-1} As, its transpose As^T Msp^{-T}, or its adjoint.  The
    // transposed sequence (sweeps first, then the SpMV with As^T) has graphs of its own; T and H share them, the
    // conjugations of H sit in the copies around the graph.
    int op = LSFC_OP_N;
    lsfc::BlockTriT tt{};              // the tables of the transposed apply, built by the first set_op(T | H)
    lsfc::CapturedSeq seq_t;
    std::unique_ptr<lsfc::CapturedSeq[]> bseq_t;
    void drop_group_graphs() {
        bseq.reset(new lsfc::CapturedSeq[lsfc::LSFC_MAX_BATCH + 1]);
        bseq_t.reset(new lsfc::CapturedSeq[lsfc::LSFC_MAX_BATCH + 1]);
    }
    lsfc_precond() { drop_group_graphs(); }
    ~lsfc_precond() { lsfc::blocktri_destroy(bt); }
};

namespace lsfc {

static void enqueue_all(lsfc_precond* pc, hipStream_t st) {
    const int N = (int)pc->N;
    hipLaunchKernelGGL(k_spmv_gather<8>, dim3((unsigned)(((int64_t)N * 8 + 255) / 256)), dim3(256), 0, st, pc->a_rowptr.p, pc->a_col.p, pc->a_val.p,
                       pc->rgather.p, pc->rscale.p, pc->vin.p, pc->y0.p, N);
    if (pc->bt) { blocktri_enqueue(pc->bt, pc->y0.p, pc->vout.p, st); return; }
    launch_factor(pc->L, pc->y0.p, pc->z.p, st);
    launch_factor(pc->U, pc->z.p, pc->w.p, st);
    hipLaunchKernelGGL(k_scatter, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, pc->w.p, pc->cscatter.p, pc->vout.p, N);
}

// the transposed sequence of a block-tridiagonal object: vout <- As^T (Msp^{-T} vin), the sweeps first
static void enqueue_all_t(lsfc_precond* pc, hipStream_t st) {
    const int N = (int)pc->N;
    blocktri_enqueue(pc->bt, pc->vin.p, pc->y0.p, st, true);
    hipLaunchKernelGGL(k_spmv_gather<8>, dim3((unsigned)(((int64_t)N * 8 + 255) / 256)), dim3(256), 0, st, pc->tt.rowptr, pc->tt.col, pc->tt.as_val,
                       (const int*)nullptr, (const double*)nullptr, (const cplx*)pc->y0.p, pc->vout.p, N);
}

// v (device, N complex) <- Msp^{-1} (As v), or what pc->op makes of it, stream-ordered on `st`
static void precond_apply_dev(lsfc_precond* pc, cplx* v, hipStream_t st) {
    const size_t bytes = (size_t)pc->N * sizeof(cplx);
    if (pc->op != LSFC_OP_N) {
        const bool conj = pc->op == LSFC_OP_H;
        GroupPtrs g{}; g.v[0] = v;
        const dim3 cgrid((unsigned)((pc->N + 255) / 256), 1u);
        if (conj) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_group_copy<true, true>), cgrid, dim3(256), 0, st, g, pc->vin.p, pc->N);
        else LSFC_HIP(hipMemcpyAsync(pc->vin.p, v, bytes, hipMemcpyDeviceToDevice, st));
        pc->seq_t.replay(st, 0, [&](hipStream_t s) { enqueue_all_t(pc, s); });
        if (conj) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_group_copy<false, true>), cgrid, dim3(256), 0, st, g, pc->vout.p, pc->N);
        else LSFC_HIP(hipMemcpyAsync(v, pc->vout.p, bytes, hipMemcpyDeviceToDevice, st));
        LSFC_HIP(hipGetLastError());
        return;
    }
    LSFC_HIP(hipMemcpyAsync(pc->vin.p, v, bytes, hipMemcpyDeviceToDevice, st));
    pc->seq.replay(st, 0, [&](hipStream_t s) { enqueue_all(pc, s); });
    LSFC_HIP(hipMemcpyAsync(v, pc->vout.p, bytes, hipMemcpyDeviceToDevice, st));
}

// the fixed part of a group apply, on internal buffers only: SpMV for R members, then the group sweep
static void enqueue_group(lsfc_precond* pc, int R, hipStream_t st) {
    const int N = (int)pc->N;
    const dim3 grid((unsigned)(((int64_t)N * 8 + 255) / 256)), block(256);
    dispatch<1, LSFC_MAX_BATCH>(R, "preconditioner group apply", [&](auto rc) {
        hipLaunchKernelGGL(k_spmv_batch<decltype(rc)::value>, grid, block, 0, st, pc->a_rowptr.p, pc->a_col.p, pc->a_val.p, (const cplx*)pc->bvin.p, pc->by0.p, N);
    });
    blocktri_enqueue_batch(pc->bt, R, pc->by0.p, pc->bvout.p, st);
}

// the same for the transposed apply: the group sweep first, then the SpMV with As^T for R members
static void enqueue_group_t(lsfc_precond* pc, int R, hipStream_t st) {
    const int N = (int)pc->N;
    const dim3 grid((unsigned)(((int64_t)N * 8 + 255) / 256)), block(256);
    blocktri_enqueue_batch(pc->bt, R, pc->bvin.p, pc->by0.p, st, true);
    dispatch<1, LSFC_MAX_BATCH>(R, "preconditioner group apply", [&](auto rc) {
        hipLaunchKernelGGL(k_spmv_batch<decltype(rc)::value>, grid, block, 0, st, pc->tt.rowptr, pc->tt.col, pc->tt.as_val, (const cplx*)pc->by0.p, pc->bvout.p, N);
    });
}

// one group of R <= LSFC_MAX_BATCH vectors of a block-tridiagonal object
static void precond_apply_group(lsfc_precond* pc, cplx* const* v, int R, hipStream_t st) {
    if (R > pc->bcap) {
        // work space on first use (and when a larger group comes): the captured graphs hold the old addresses
        LSFC_HIP(hipDeviceSynchronize());
        pc->drop_group_graphs();
        const size_t n = (size_t)R * (size_t)pc->N;
        pc->bvin.alloc(n); pc->by0.alloc(n); pc->bvout.alloc(n);
        pc->bwork_bytes = (int64_t)(3 * n * sizeof(cplx)) + blocktri_batch_reserve(pc->bt, R);
        pc->bcap = R;
    }
    GroupPtrs g{};
    for (int r = 0; r < R; ++r) g.v[r] = v[r];
    const dim3 cgrid((unsigned)((pc->N + 255) / 256), (unsigned)R);
    const bool conj = pc->op == LSFC_OP_H;
    if (conj) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_group_copy<true, true>), cgrid, dim3(256), 0, st, g, pc->bvin.p, pc->N);
    else hipLaunchKernelGGL(k_group_copy<true>, cgrid, dim3(256), 0, st, g, pc->bvin.p, pc->N);
    if (pc->op == LSFC_OP_N) pc->bseq[R].replay(st, R, [&](hipStream_t s) { enqueue_group(pc, R, s); });
    else pc->bseq_t[R].replay(st, R, [&](hipStream_t s) { enqueue_group_t(pc, R, s); });
    if (conj) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_group_copy<false, true>), cgrid, dim3(256), 0, st, g, pc->bvout.p, pc->N);
    else hipLaunchKernelGGL(k_group_copy<false>, cgrid, dim3(256), 0, st, g, pc->bvout.p, pc->N);
    LSFC_HIP(hipGetLastError());
    ++pc->bsweeps; pc->bvectors += R; pc->blargest = std::max<int64_t>(pc->blargest, R);
}

void precond_apply_batch_dev(lsfc_precond* pc, cplx* const* v, int cnt, hipStream_t st) {
    if (!pc->bt) { for (int j = 0; j < cnt; ++j) precond_apply_dev(pc, v[j], st); return; }
    for (int j0 = 0; j0 < cnt; j0 += LSFC_MAX_BATCH) precond_apply_group(pc, v + j0, std::min(LSFC_MAX_BATCH, cnt - j0), st);
}

int64_t precond_size(const lsfc_precond* pc) { return pc->N; }
int precond_op(const lsfc_precond* pc) { return pc->op; }

// the preconditioner hand-off of the Krylov solvers (plan.hpp)
void plan_check_precond_op(const lsfc_plan* p, lsfc_precond_fn fn, void* precond_user, const char* who) {
    if (fn != &lsfc_precond_callback) return;
    static const char* const names[] = {"LSFC_OP_N", "LSFC_OP_T", "LSFC_OP_H"};
    const int pop = precond_user ? precond_op((const lsfc_precond*)precond_user) : LSFC_OP_N;
    LSFC_REQUIRE(pop == p->op, "%s%sthe library's preconditioner object is set to %s and approximates the inverse of that form of M, the plan is set to %s: "
                 "lsfc_precond_set_op and lsfc_plan_set_op must agree", who ? who : "", who ? ": " : "", names[pop], names[p->op]);
}

Precond::Precond(lsfc_precond_fn f, void* u, bool dev, bool meet, int64_t n, const char* who)
    : fn(f), user(u), on_device(dev), own(meet && dev && f == &lsfc_precond_callback), N(n) {
    const int64_t have = own && user ? precond_size((lsfc_precond*)user) : -1;
    if (own) LSFC_REQUIRE(have == N, "%s%spreconditioner: size mismatch (%lld vs %lld)", who ? who : "", who ? ": " : "", (long long)N, (long long)have);
}

void Precond::apply(cplx* const* v, size_t cnt, cplx* pinned, hipStream_t st) const {
    if (!fn) return;
    if (own) { precond_apply_batch_dev((lsfc_precond*)user, v, (int)cnt, st); return; }
    for (size_t j = 0; j < cnt; ++j) {
        if (!on_device) {
            LSFC_HIP(hipMemcpyAsync(pinned, v[j], (size_t)N * sizeof(cplx), hipMemcpyDeviceToHost, st));
            LSFC_HIP(hipStreamSynchronize(st));
        }
        const int rc = fn(user, (double*)(on_device ? v[j] : pinned), N);
        if (rc != 0) fail(LSFC_EINVAL, "preconditioner callback returned %d", rc);
        // (whatever next goes into the pinned vector is ordered after this copy on st)
        if (!on_device) LSFC_HIP(hipMemcpyAsync(v[j], pinned, (size_t)N * sizeof(cplx), hipMemcpyHostToDevice, st));
    }
}

// loads this translation unit's code object on the current device (pruned.hip: pruned_warmup -- every code object of the library is
// resident before the first transfer or pass of a process exists; DESIGN 3, "The round-2 first-apply GPU fault")
__global__ void k_warmup_precond(int* p) { if (p) *p = 0; }
void warmup_precond() {
    hipLaunchKernelGGL(k_warmup_precond, dim3(1), dim3(64), 0, 0, (int*)nullptr);
    LSFC_HIP(hipGetLastError());
}

// nrhs HOST vectors back to back, a group at a time through the staging buffer: copy up, apply(staged vectors, how many),
// copy down; synchronised on return
template <class F> static void apply_staged(lsfc_precond* pc, cplx* v, int64_t nrhs, F&& apply) {
    const int64_t N = pc->N, grp = std::min<int64_t>(nrhs, LSFC_MAX_BATCH);
    if (pc->hstage.n < (size_t)(grp * N)) pc->hstage.alloc((size_t)(grp * N));
    for (int64_t j0 = 0; j0 < nrhs; j0 += grp) {
        const int cnt = (int)std::min<int64_t>(grp, nrhs - j0);
        const size_t bytes = (size_t)cnt * (size_t)N * sizeof(cplx);
        LSFC_HIP(hipMemcpyAsync(pc->hstage.p, v + j0 * N, bytes, hipMemcpyHostToDevice, pc->stream));
        apply(pc->hstage.p, cnt);
        LSFC_HIP(hipMemcpyAsync(v + j0 * N, pc->hstage.p, bytes, hipMemcpyDeviceToHost, pc->stream));
    }
    LSFC_HIP(hipStreamSynchronize(pc->stream));
}

} // namespace lsfc

using namespace lsfc;

extern "C" {

int lsfc_precond_create(lsfc_precond** out, int64_t N,
                        const int64_t* As_rowptr, const int64_t* As_col, const double* As_val,
                        const int64_t* L_rowptr, const int64_t* L_col, const double* L_val,
                        const int64_t* U_rowptr, const int64_t* U_col, const double* U_val,
                        const int64_t* row_gather, const int64_t* col_scatter, const double* row_scale, int device) {
    return guarded([&] {
        LSFC_REQUIRE(out, "NULL argument"); *out = nullptr;
        LSFC_REQUIRE(N >= 1 && N < ((int64_t)1 << 31), "preconditioner: N out of range");
        LSFC_REQUIRE(As_rowptr && As_col && As_val && L_rowptr && L_col && L_val && U_rowptr && U_col && U_val, "NULL argument");
        select_device(device, "preconditioner apply");
        pruned_warmup(device);                             // every code object of the library resident before any work of this process is queued
        std::unique_ptr<lsfc_precond> pc(new lsfc_precond());
        pc->device = device; pc->N = N;
        // As: CSR, 32-bit columns on the device
        {
            const int64_t nnz = As_rowptr[N];
            std::vector<int> c((size_t)nnz);
            for (int64_t e = 0; e < nnz; ++e) { LSFC_REQUIRE(As_col[e] >= 0 && As_col[e] < N, "As: column index out of range"); c[(size_t)e] = (int)As_col[e]; }
            pc->a_rowptr.alloc((size_t)N + 1); pc->a_col.alloc((size_t)nnz); pc->a_val.alloc((size_t)nnz);
            LSFC_HIP(hipMemcpy(pc->a_rowptr.p, As_rowptr, ((size_t)N + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
            if (nnz) {
                LSFC_HIP(hipMemcpy(pc->a_col.p, c.data(), (size_t)nnz * sizeof(int), hipMemcpyHostToDevice));
                LSFC_HIP(hipMemcpy(pc->a_val.p, As_val, (size_t)nnz * sizeof(cplx), hipMemcpyHostToDevice));
            }
        }
        auto perm_up = [&](DevBuf<int>& dev, const int64_t* p, const char* what) {
            std::vector<int> h((size_t)N); std::vector<char> seen((size_t)N, 0);
            for (int64_t i = 0; i < N; ++i) {
                const int64_t v = p ? p[i] : i;
                LSFC_REQUIRE(v >= 0 && v < N && !seen[(size_t)v], "preconditioner: %s is not a permutation", what);
                seen[(size_t)v] = 1; h[(size_t)i] = (int)v;
            }
            dev.alloc((size_t)N);
            LSFC_HIP(hipMemcpy(dev.p, h.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice));
        };
        perm_up(pc->rgather, row_gather, "row_gather");
        perm_up(pc->cscatter, col_scatter, "col_scatter");
        if (row_scale) { pc->rscale.alloc((size_t)N); LSFC_HIP(hipMemcpy(pc->rscale.p, row_scale, (size_t)N * sizeof(double), hipMemcpyHostToDevice)); }
        build_factor(pc->L, N, L_rowptr, L_col, L_val, true);
        build_factor(pc->U, N, U_rowptr, U_col, U_val, false);
        for (DevBuf<cplx>* b : { &pc->vin, &pc->y0, &pc->z, &pc->w, &pc->vout }) { b->alloc((size_t)N); LSFC_HIP(hipMemset(b->p, 0, b->bytes())); }
        pc->launches = 2;
        for (const TriFactor* F : { &pc->L, &pc->U }) for (const auto& sg : F->segs) {
            if (sg.kind == 3) { const int nb = (F->runs[(size_t)sg.l0].R + RUN_BLOCK - 1) / RUN_BLOCK; pc->launches += 2 * nb; }
            else pc->launches += sg.kind == 2 ? 2 : 1;
        }
        *out = pc.release();
    });
}

int lsfc_precond_destroy(lsfc_precond* pc) {
    return guarded([&] { if (pc) { (void)hipSetDevice(pc->device); (void)hipDeviceSynchronize(); delete pc; } });
}

int lsfc_precond_set_stream(lsfc_precond* pc, void* stream) {
    return guarded([&] { LSFC_REQUIRE(pc, "NULL preconditioner"); pc->stream = (hipStream_t)stream; });
}

int lsfc_precond_set_op(lsfc_precond* pc, int op) {
    return guarded([&] {
        LSFC_REQUIRE(pc, "NULL preconditioner");
        LSFC_REQUIRE(op == LSFC_OP_N || op == LSFC_OP_T || op == LSFC_OP_H, "bad op %d (LSFC_OP_N, LSFC_OP_T or LSFC_OP_H)", op);
        LSFC_REQUIRE(op == LSFC_OP_N || pc->bt, "the transposed and the adjoint apply need a block-tridiagonal object (lsfc_precond_create_blocktri / "
                     "_from_plan); this one holds the host's LU factors (lsfc_precond_create), whose transposed level-scheduled solves are not offered");
        if (op != LSFC_OP_N && !pc->tt.rowptr) {
            LSFC_HIP(hipSetDevice(pc->device));
            pc->tt = blocktri_transpose_tables(pc->bt, pc->a_val.p);
        }
        pc->op = op;
    });
}

int lsfc_precond_get_op(const lsfc_precond* pc, int* op, int64_t* table_bytes) {
    return guarded([&] {
        LSFC_REQUIRE(pc && op, "NULL argument");
        *op = pc->op;
        if (table_bytes) *table_bytes = pc->tt.bytes;
    });
}

int lsfc_precond_apply(lsfc_precond* pc, double* v, int memspace) {
    return guarded([&] {
        LSFC_REQUIRE(pc && v, "NULL argument");
        LSFC_REQUIRE(memspace == LSFC_MEM_HOST || memspace == LSFC_MEM_DEVICE, "bad memspace %d", memspace);
        LSFC_HIP(hipSetDevice(pc->device));
        if (memspace == LSFC_MEM_DEVICE) { precond_apply_dev(pc, (cplx*)v, pc->stream); return; }
        apply_staged(pc, (cplx*)v, 1, [&](cplx* staged, int) { precond_apply_dev(pc, staged, pc->stream); });
    });
}

int lsfc_precond_apply_batch(lsfc_precond* pc, double* v, int64_t nrhs, int memspace) {
    return guarded([&] {
        LSFC_REQUIRE(pc && v, "NULL argument");
        LSFC_REQUIRE(nrhs >= 1 && nrhs < ((int64_t)1 << 31), "nrhs = %lld: need at least one right-hand side", (long long)nrhs);
        LSFC_REQUIRE(memspace == LSFC_MEM_HOST || memspace == LSFC_MEM_DEVICE, "bad memspace %d", memspace);
        LSFC_HIP(hipSetDevice(pc->device));
        std::vector<cplx*> ptr((size_t)nrhs);
        auto apply = [&](cplx* dev, int cnt) {              // cnt device vectors back to back
            for (int j = 0; j < cnt; ++j) ptr[(size_t)j] = dev + (int64_t)j * pc->N;
            precond_apply_batch_dev(pc, ptr.data(), cnt, pc->stream);
        };
        if (memspace == LSFC_MEM_DEVICE) apply((cplx*)v, (int)nrhs); else apply_staged(pc, (cplx*)v, nrhs, apply);
    });
}

int lsfc_precond_batch_info(const lsfc_precond* pc, int64_t out[4]) {
    return guarded([&] {
        LSFC_REQUIRE(pc && out, "NULL argument");
        out[0] = pc->bsweeps; out[1] = pc->bvectors; out[2] = pc->blargest; out[3] = pc->bwork_bytes;
    });
}

/* lsfc_precond_fn-compatible entry: opts.precond = lsfc_precond_callback, opts.precond_user = pc,
 * opts.precond_on_device = 1 (v is the device-resident Krylov vector; work is enqueued on pc's stream). */
int lsfc_precond_callback(void* user, double* v, int64_t n) {
    lsfc_precond* pc = (lsfc_precond*)user;
    if (!pc || n != pc->N) { set_last_error("preconditioner callback: size mismatch (%lld vs %lld)", (long long)n, pc ? (long long)pc->N : -1LL); return 1; }
    return lsfc_precond_apply(pc, v, LSFC_MEM_DEVICE) == LSFC_OK ? 0 : 1;
}

int lsfc_precond_stats(const lsfc_precond* pc, int64_t* levels_L, int64_t* levels_U, int64_t* launches) {
    return guarded([&] {
        LSFC_REQUIRE(pc, "NULL preconditioner");
        if (levels_L) *levels_L = pc->bt ? blocktri_info(pc->bt).K : pc->L.nlevels;
        if (levels_U) *levels_U = pc->bt ? blocktri_info(pc->bt).K : pc->U.nlevels;
        if (launches) *launches = pc->launches;
    });
}

int lsfc_precond_schedule(const lsfc_precond* pc, int factor, int64_t out[10]) {
    return guarded([&] {
        LSFC_REQUIRE(pc && out, "NULL argument");
        LSFC_REQUIRE(factor == 0 || factor == 1, "bad factor %d (0 = L, 1 = U)", factor);
        LSFC_REQUIRE(!pc->bt, "a block-tridiagonal preconditioner has no level schedule (see lsfc_precond_blocktri_info)");
        const lsfc::TriFactor& F = factor == 0 ? pc->L : pc->U;
        for (int i = 0; i < 10; ++i) out[i] = F.sched[i];
    });
}

} // extern "C"

// ---- block-tridiagonal route: factorised on the device (blocktri.hip) ----------------------------------------------

namespace lsfc {

// the object from DEVICE arrays of one shared pattern; the current device is `device`
static lsfc_precond* create_blocktri_dev(int64_t N, int64_t K, const int64_t* rowptr, const int64_t* col, const cplx* As, const cplx* Msp, int device,
                                         int prec, int pivoting) {
    std::unique_ptr<lsfc_precond> pc(new lsfc_precond());
    pc->device = device; pc->N = N;
    pc->bt = blocktri_factor(N, K, rowptr, col, Msp, prec, pivoting);
    const int64_t nnz = blocktri_nnz(pc->bt);
    pc->a_rowptr.alloc((size_t)N + 1); pc->a_col.alloc((size_t)nnz); pc->a_val.alloc((size_t)nnz);
    LSFC_HIP(hipMemcpy(pc->a_rowptr.p, rowptr, ((size_t)N + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice));
    LSFC_HIP(hipMemcpy(pc->a_col.p, blocktri_col32(pc->bt), (size_t)nnz * sizeof(int), hipMemcpyDeviceToDevice));
    LSFC_HIP(hipMemcpy(pc->a_val.p, As, (size_t)nnz * sizeof(cplx), hipMemcpyDeviceToDevice));
    for (DevBuf<cplx>* b : { &pc->vin, &pc->y0, &pc->vout }) { b->alloc((size_t)N); LSFC_HIP(hipMemset(b->p, 0, b->bytes())); }
    pc->launches = 1 + (int)blocktri_info(pc->bt).launches;
    LSFC_HIP(hipDeviceSynchronize());
    return pc.release();
}

// the options of the two _opts constructors, checked before any device call; NULL: fp64 storage, no pivoting
struct BtOpts { int prec, pivoting; };
static BtOpts checked_opts(const lsfc_blocktri_opts* o) {
    if (!o) return BtOpts{LSFC_PRECOND_INV_F64, LSFC_PRECOND_PIVOT_NONE};
    LSFC_REQUIRE(o->inverse_precision == LSFC_PRECOND_INV_F64 || o->inverse_precision == LSFC_PRECOND_INV_F32,
                 "bad inverse_precision %d (LSFC_PRECOND_INV_F64 or _F32)", o->inverse_precision);
    LSFC_REQUIRE(o->pivoting == LSFC_PRECOND_PIVOT_NONE || o->pivoting == LSFC_PRECOND_PIVOT_PARTIAL || o->pivoting == LSFC_PRECOND_PIVOT_AUTO,
                 "bad pivoting %d (LSFC_PRECOND_PIVOT_NONE, _PARTIAL or _AUTO)", o->pivoting);
    for (int i = 0; i < 6; ++i) LSFC_REQUIRE(o->reserved[i] == 0, "lsfc_blocktri_opts: reserved[%d] = %d must be zero", i, o->reserved[i]);
    return BtOpts{o->inverse_precision, o->pivoting};
}
static lsfc_blocktri_opts opts_of_precision(int inverse_precision) {
    lsfc_blocktri_opts o{};
    o.inverse_precision = inverse_precision; o.pivoting = LSFC_PRECOND_PIVOT_NONE;
    return o;
}

} // namespace lsfc

extern "C" {

int lsfc_precond_create_blocktri(lsfc_precond** out, int64_t N, int64_t nblocks, const int64_t* rowptr, const int64_t* col,
                                 const double* As_val, const double* Msp_val, int memspace, int device) {
    return lsfc_precond_create_blocktri_prec(out, N, nblocks, rowptr, col, As_val, Msp_val, memspace, device, LSFC_PRECOND_INV_F64);
}

int lsfc_precond_create_blocktri_prec(lsfc_precond** out, int64_t N, int64_t nblocks, const int64_t* rowptr, const int64_t* col,
                                      const double* As_val, const double* Msp_val, int memspace, int device, int inverse_precision) {
    const lsfc_blocktri_opts o = opts_of_precision(inverse_precision);
    return lsfc_precond_create_blocktri_opts(out, N, nblocks, rowptr, col, As_val, Msp_val, memspace, device, &o);
}

int lsfc_precond_create_blocktri_opts(lsfc_precond** out, int64_t N, int64_t nblocks, const int64_t* rowptr, const int64_t* col,
                                      const double* As_val, const double* Msp_val, int memspace, int device, const lsfc_blocktri_opts* opts) {
    return guarded([&] {
        LSFC_REQUIRE(out, "NULL argument"); *out = nullptr;
        const BtOpts bo = checked_opts(opts);
        const int prec = bo.prec, piv = bo.pivoting;
        LSFC_REQUIRE(rowptr && col && As_val && Msp_val, "NULL argument");
        LSFC_REQUIRE(memspace == LSFC_MEM_HOST || memspace == LSFC_MEM_DEVICE, "bad memspace %d", memspace);
        LSFC_REQUIRE(N >= 1 && N < ((int64_t)1 << 31), "preconditioner: N out of range");
        LSFC_REQUIRE(nblocks >= 1 && N % nblocks == 0, "block-tridiagonal preconditioner: N = %lld is not divisible by nblocks = %lld", (long long)N, (long long)nblocks);
        select_device(device, "preconditioner");
        pruned_warmup(device);
        blocktri_require_memory(N, nblocks, 0.0, "lsfc_precond_create_blocktri", prec, piv);   // from the dimensions and options alone, before any array is read
        if (memspace == LSFC_MEM_DEVICE) { *out = create_blocktri_dev(N, nblocks, rowptr, col, (const cplx*)As_val, (const cplx*)Msp_val, device, prec, piv); return; }
        const int64_t nnz = rowptr[N];
        LSFC_REQUIRE(nnz >= 0, "block-tridiagonal preconditioner: rowptr[N] is negative");
        DevBuf<int64_t> drp, dcol; DevBuf<cplx> das, dmsp;
        drp.alloc((size_t)N + 1); dcol.alloc((size_t)nnz); das.alloc((size_t)nnz); dmsp.alloc((size_t)nnz);
        LSFC_HIP(hipMemcpy(drp.p, rowptr, ((size_t)N + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
        if (nnz) {
            LSFC_HIP(hipMemcpy(dcol.p, col, (size_t)nnz * sizeof(int64_t), hipMemcpyHostToDevice));
            LSFC_HIP(hipMemcpy(das.p, As_val, (size_t)nnz * sizeof(cplx), hipMemcpyHostToDevice));
            LSFC_HIP(hipMemcpy(dmsp.p, Msp_val, (size_t)nnz * sizeof(cplx), hipMemcpyHostToDevice));
        }
        *out = create_blocktri_dev(N, nblocks, drp.p, dcol.p, das.p, dmsp.p, device, prec, piv);
    });
}

int lsfc_precond_create_from_plan(lsfc_precond** out, lsfc_plan* plan) { return lsfc_precond_create_from_plan_prec(out, plan, LSFC_PRECOND_INV_F64); }

int lsfc_precond_create_from_plan_prec(lsfc_precond** out, lsfc_plan* plan, int inverse_precision) {
    const lsfc_blocktri_opts o = opts_of_precision(inverse_precision);
    return lsfc_precond_create_from_plan_opts(out, plan, &o);
}

int lsfc_precond_create_from_plan_opts(lsfc_precond** out, lsfc_plan* plan, const lsfc_blocktri_opts* opts) {
    return guarded([&] {
        LSFC_REQUIRE(out, "NULL argument"); *out = nullptr;
        const BtOpts bo = checked_opts(opts);
        const int prec = bo.prec, piv = bo.pivoting;
        LSFC_REQUIRE(plan, "NULL plan");
        LSFC_REQUIRE(!plan->dist && !plan->multi, "block-tridiagonal preconditioner: not available on a distributed or multi-device plan");
        const int64_t n = plan->dims[0], m = plan->dims[1], l = plan->ndim == 2 ? 1 : plan->dims[2];
        const int64_t N = n * m * l, K = plan->ndim == 2 ? m : l;
        int64_t nnz = 0;
        if (int rc = lsfc_sparsify_pattern(n, m, l, &nnz, nullptr, nullptr, nullptr)) fail(rc, "%s", lsfc_last_error());
        select_device(plan->device, "preconditioner");
        pruned_warmup(plan->device);
        blocktri_require_memory(N, K, (double)nnz * 40.0, "lsfc_precond_create_from_plan", prec, piv);
        DevBuf<int64_t> drp, dcol; DevBuf<cplx> das, dmsp;
        drp.alloc((size_t)N + 1); dcol.alloc((size_t)nnz); das.alloc((size_t)nnz); dmsp.alloc((size_t)nnz);
        if (int rc = lsfc_sparsify_build(plan, drp.p, dcol.p, (double*)das.p, nullptr, (double*)dmsp.p, nullptr, LSFC_MEM_DEVICE)) fail(rc, "%s", lsfc_last_error());
        *out = create_blocktri_dev(N, K, drp.p, dcol.p, das.p, dmsp.p, plan->device, prec, piv);
    });
}

int lsfc_precond_blocktri_info(const lsfc_precond* pc, int64_t out[6], double* min_pivot_ratio) {
    return guarded([&] {
        LSFC_REQUIRE(pc && out, "NULL argument");
        LSFC_REQUIRE(pc->bt, "not a block-tridiagonal preconditioner (made by lsfc_precond_create)");
        const BlockTriInfo i = blocktri_info(pc->bt);
        out[0] = i.K; out[1] = i.b; out[2] = i.factor_bytes; out[3] = pc->launches; out[4] = i.factor_us; out[5] = i.pivoting;
        if (min_pivot_ratio) *min_pivot_ratio = i.min_pivot_ratio;
    });
}

int lsfc_precond_inverse_precision(const lsfc_precond* pc, int* precision) {
    return guarded([&] {
        LSFC_REQUIRE(pc && precision, "NULL argument");
        LSFC_REQUIRE(pc->bt, "not a block-tridiagonal preconditioner (made by lsfc_precond_create)");
        *precision = blocktri_precision(pc->bt);
    });
}

int lsfc_precond_blocktri_get_block(const lsfc_precond* pc, int64_t k, double* out, int64_t capacity_complex) {
    return guarded([&] {
        LSFC_REQUIRE(pc && out, "NULL argument");
        LSFC_REQUIRE(pc->bt, "not a block-tridiagonal preconditioner (made by lsfc_precond_create)");
        const BlockTriInfo i = blocktri_info(pc->bt);
        LSFC_REQUIRE(k >= 0 && k < i.K, "block %lld out of range (have %lld)", (long long)k, (long long)i.K);
        LSFC_REQUIRE(capacity_complex >= i.b * i.b, "capacity %lld is less than the %lld entries of a block", (long long)capacity_complex, (long long)(i.b * i.b));
        LSFC_HIP(hipSetDevice(pc->device));
        blocktri_get_block(pc->bt, k, (cplx*)out);
    });
}

int lsfc_precond_blocktri_get_pivots(const lsfc_precond* pc, int64_t k, int64_t* perm, int64_t capacity) {
    return guarded([&] {
        LSFC_REQUIRE(pc && perm, "NULL argument");
        LSFC_REQUIRE(pc->bt, "not a block-tridiagonal preconditioner (made by lsfc_precond_create)");
        const BlockTriInfo i = blocktri_info(pc->bt);
        LSFC_REQUIRE(k >= 0 && k < i.K, "block %lld out of range (have %lld)", (long long)k, (long long)i.K);
        LSFC_REQUIRE(capacity >= i.b, "capacity %lld is less than the %lld rows of a block", (long long)capacity, (long long)i.b);
        LSFC_HIP(hipSetDevice(pc->device));
        blocktri_get_pivots(pc->bt, k, perm);
    });
}

} // extern "C"
