// Left-preconditioned BiCGStab(l) on the device, arithmetic of IterativeSolvers.jl bicgstabl! with one departure: the
// shadow residual is the preconditioned initial residual (or the caller's vector), not rand.  2 l + 3 work vectors of N
// complex whatever the iteration count: rs[0..l], us[0..l], the shadow residual.
//
// Every logical step of a cycle is ONE launch that reads each vector it touches once:
//   k_bicg_u      us[i] = rs[i] - beta us[i], i <= j           (sums the partials of rho itself, forms beta = rho / sigma)
//   k_bicg_rx     rs[i] -= alpha us[i+1], i <= j; x += alpha us[0]   (sums the partials of sigma, forms alpha = rho / sigma)
//   k_gram        all (l+1)(l+2)/2 entries of G = rs' rs in one pass over the l + 1 residual vectors
//   k_mr_solve    one wave: G from its partials, the exit G[0,0] <= tol^2, gamma = G[1:,1:] \ G[1:,0] (LU, partial pivoting)
//   k_mr_update   us[0] -= sum gamma_i us[i+1]; x += sum gamma_i rs[i]; rs[0] -= sum gamma_i rs[i+1]; partials of |rs[0]|^2
// rho, sigma, beta, alpha, gamma and a status word live in device memory; the host reads them (with G and the residual norm)
// once per cycle.  Reductions: the fixed-order tree of reduce.hpp, so two solves of the same input are bitwise equal.
// An update whose scalar is zero where it divides, or not finite, is skipped by every block (each block forms the scalar
// from the same partials in the same order), the status word names it, and all later updates are skipped too: x and rs[0]
// stay the last finite, mutually consistent pair.
//
// Lock step (lsfc_bicgstabl_batch): every kernel has a member dimension, blockIdx.y = position in the launch's member list
// (struct Members, passed by value).  Member m owns its 2 l + 3 work vectors, a block of S_COUNT scalars, a block of
// P_SLOTS * RED_BLOCKS partials and an entry of the tol^2 array; inside a member the block count, the grid-stride
// mapping, the slots and the order of summation do not depend on the other members, so a member's bits are those of its
// solve alone.  The host reads all scalar blocks in one copy per cycle and drops the members that have stopped from
// the list of the next cycle.  lsfc_bicgstabl is the call with one member.
//
// The cycle is written once, over RANKS (struct Rank, bicgstabl_run): one rank is the plan itself -- the launches above, nothing
// else -- and the P ranks of a single-process multi-device plan (lsfc_bicgstabl_multi) each hold the z slab of every vector on their own device (the
// team form, k_rank_sum below: sums completed across the ranks in device memory, ordered by events, no host in between).
#include "plan.hpp"
#include "krylov_blas.hpp"
#include "reduce.hpp"
#include "team.hpp"
#include <algorithm>
#include <cmath>
#include <type_traits>
#include <vector>

namespace lsfc {
namespace {

constexpr int LMAX = 8, NVMAX = LMAX + 1;
// device scalars (cplx each)
enum { S_RHO = 0, S_SIGMA = 1, S_BETA = 2, S_ALPHA = 3, S_STATUS = 4 /* (code, cycle) */, S_RES = 5, S_GAMMA = 6 /* LMAX */,
       S_G = 16 /* NVMAX * NVMAX, row-major */, S_COUNT = 16 + NVMAX * NVMAX };
enum { ST_OK = 0, ST_EXHAUSTED = 1, ST_RHO = 2, ST_SIGMA = 3, ST_BETA = 4, ST_ALPHA = 5, ST_GAMMA = 6, ST_RESIDUAL = 7 };
static_assert(ST_RHO == LSFC_BICG_RHO && ST_SIGMA == LSFC_BICG_SIGMA && ST_BETA == LSFC_BICG_BETA && ST_ALPHA == LSFC_BICG_ALPHA &&
              ST_GAMMA == LSFC_BICG_GAMMA && ST_RESIDUAL == LSFC_BICG_RESIDUAL, "the public codes are the status words");
const char* const ST_NAME[] = { "", "", "rho is not finite", "sigma is zero or not finite", "beta = rho / sigma is not finite",
                                "alpha = rho / sigma is not finite", "gamma (singular or non-finite Gram matrix)",
                                "the residual norm is not finite" };
// partial slots (RED_BLOCKS entries each): rho, sigma, |rs[0]|^2, then the Gram entries
enum { P_RHO = 0, P_SIGMA = 1, P_NORM = 2, P_GRAM = 3, P_SLOTS = 3 + NVMAX * (NVMAX + 1) / 2 };

__device__ __forceinline__ bool fin(cplx a) { return isfinite(a.x) && isfinite(a.y); }
__device__ __forceinline__ cplx cmul(cplx a, cplx b) { return make_double2(fma(a.x, b.x, -a.y * b.y), fma(a.x, b.y, a.y * b.x)); }
__device__ __forceinline__ cplx cdiv(cplx a, cplx b) {
    const double d = fma(b.x, b.x, b.y * b.y);
    return make_double2(fma(a.x, b.x, a.y * b.y) / d, fma(a.y, b.x, -a.x * b.y) / d);
}

// The members of one launch and where their data lives; by value in every kernel of the solve, member = m[blockIdx.y].
// Member m: work vectors work + m wstride (rs[0..l], us[0..l], the shadow residual, n apart), x + m n,
// scal + m S_COUNT, partial + m P_SLOTS RED_BLOCKS, tol2[m].
struct Members {
    cplx* work; cplx* x; cplx* scal; cplx* partial; const double* tol2;
    cplx* table; int rank, nranks;                       // the team form only (below)
    int64_t wstride, n;
    int m[KRYLOV_NRHS_MAX];
};
__device__ __forceinline__ cplx* m_work(const Members& B, int m) { return B.work + (int64_t)m * B.wstride; }
__device__ __forceinline__ cplx* m_scal(const Members& B, int m) { return B.scal + (int64_t)m * S_COUNT; }
__device__ __forceinline__ cplx* m_partial(const Members& B, int m) { return B.partial + (int64_t)m * (P_SLOTS * RED_BLOCKS); }

// The team form (TEAM; lsfc_bicgstabl_multi, on a multi-device plan): the vectors are cut into the z slabs of P ranks, every rank runs
// the kernels below on its slab with its own scalars, partials and tol^2 (one member), and a sum is completed in two levels.
// k_rank_sum reduces the nb partials of a slot to the RANK SUM, entry (slot, rank) of the rank's table; the rank copies it
// into the same entry of the table of every other rank; the kernel that consumes the sum adds the P entries in rank order.
// Every rank forms every scalar from the same numbers in the same order, so all ranks skip alike and their status words agree.
// table[r * P_SLOTS + slot]: the slots of one reduction lie side by side in a rank's row, so one copy per pair of ranks moves them.
__global__ __launch_bounds__(64) void k_rank_sum(Members B, int slot0, int nb) {
    const int slot = slot0 + blockIdx.x;
    const cplx s = finish_in_wave(m_partial(B, B.m[0]) + (int64_t)slot * RED_BLOCKS, nb);
    if (threadIdx.x == 0) B.table[(int64_t)B.rank * P_SLOTS + slot] = s;
}
// the sum behind partial slot `slot` of member m in all lanes of the calling wave: the nb block partials in the order of
// finish_in_wave, or (TEAM) the rank sums in rank order -- with one rank that is the entry itself, the bits of the other form
template <bool TEAM>
__device__ __forceinline__ cplx slot_sum(const Members& B, int m, int slot, int nb) {
    if constexpr (!TEAM) return finish_in_wave(m_partial(B, m) + (int64_t)slot * RED_BLOCKS, nb);
    else {
        cplx acc = B.table[slot];
        for (int r = 1; r < B.nranks; ++r) { const cplx v = B.table[(int64_t)r * P_SLOTS + slot]; acc.x += v.x; acc.y += v.y; }
        return acc;
    }
}

// rs[0] = b - rs[0], in place  (initial residual from rs[0] = A x)
__global__ void k_residual(Members B, const cplx* __restrict__ ball) {
    const int m = B.m[blockIdx.y];
    cplx* y = m_work(B, m);
    sub_slice(y, ball + (int64_t)m * B.n, y, B.n);
}

// partial slot `slot`: slices of sum_i conj(a[i]) b[i], a and b the work vectors at offsets aoff and boff (dot_slice, as
// blas_dot_partial, with a member dimension: the same slices, the same order)
__global__ __launch_bounds__(RED_THREADS) void k_dot(Members B, int64_t aoff, int64_t boff, int slot) {
    __shared__ cplx sh[RED_THREADS / 64];
    const int m = B.m[blockIdx.y];
    const cplx r = dot_slice(m_work(B, m) + aoff, m_work(B, m) + boff, B.n, sh);
    if (threadIdx.x == 0) m_partial(B, m)[(int64_t)slot * RED_BLOCKS + blockIdx.x] = r;
}

// scal[S_RES] = sqrt(sum of the P_NORM partials), whatever the status: the initial norm and the norm after a breakdown
template <bool TEAM>
__global__ __launch_bounds__(64) void k_norm_finish(Members B, int nb) {
    const int m = B.m[blockIdx.y];
    const cplx s = slot_sum<TEAM>(B, m, P_NORM, nb);
    if (threadIdx.x == 0) m_scal(B, m)[S_RES] = make_double2(sqrt(s.x), 0.0);
}

// rho = sum of the P_RHO partials, beta = rho / sigma; us[i] = rs[i] - beta us[i] for i < NV (= j + 1); block 0 publishes rho, beta
template <int NV, bool TEAM>
__global__ __launch_bounds__(RED_THREADS) void k_bicg_u(Members B, int64_t uoff, int nb, int cycle) {
    __shared__ cplx bs; __shared__ int skip;
    const int m = B.m[blockIdx.y];
    const int64_t n = B.n, ld = B.n;
    const cplx* __restrict__ rs = m_work(B, m);
    cplx* __restrict__ us = m_work(B, m) + uoff;
    cplx* scal = m_scal(B, m);
    if (threadIdx.x < 64) {
        const cplx rho = slot_sum<TEAM>(B, m, P_RHO, nb);
        if (threadIdx.x == 0) {
            const cplx sg = scal[S_SIGMA]; const double st = scal[S_STATUS].x;
            const cplx beta = cdiv(rho, sg);
            int code = ST_OK;
            if (!fin(rho)) code = ST_RHO;
            else if (!fin(sg) || (sg.x == 0.0 && sg.y == 0.0)) code = ST_SIGMA;
            else if (!fin(beta)) code = ST_BETA;
            skip = (st != 0.0) || code != ST_OK; bs = beta;
            if (blockIdx.x == 0) {
                scal[S_RHO] = rho; scal[S_BETA] = beta;
                if (st == 0.0 && code != ST_OK) scal[S_STATUS] = make_double2((double)code, (double)cycle);
            }
        }
    }
    __syncthreads();
    if (skip) return;
    const cplx beta = bs;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        cplx r[NV], u[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) { r[k] = rs[(int64_t)k * ld + i]; u[k] = us[(int64_t)k * ld + i]; }
#pragma unroll
        for (int k = 0; k < NV; ++k) us[(int64_t)k * ld + i] = csubmul(r[k], beta, u[k]);
    }
}

// sigma = sum of the P_SIGMA partials, alpha = rho / sigma; rs[i] -= alpha us[i+1] for i < NV (= j + 1), x += alpha us[0];
// block 0 publishes sigma, alpha
template <int NV, bool TEAM>
__global__ __launch_bounds__(RED_THREADS) void k_bicg_rx(Members B, int64_t uoff, int nb, int cycle) {
    __shared__ cplx as; __shared__ int skip;
    const int m = B.m[blockIdx.y];
    const int64_t n = B.n, ld = B.n;
    cplx* __restrict__ rs = m_work(B, m);
    const cplx* __restrict__ us = m_work(B, m) + uoff;
    cplx* __restrict__ x = B.x + (int64_t)m * n;
    cplx* scal = m_scal(B, m);
    if (threadIdx.x < 64) {
        const cplx sg = slot_sum<TEAM>(B, m, P_SIGMA, nb);
        if (threadIdx.x == 0) {
            const cplx rho = scal[S_RHO]; const double st = scal[S_STATUS].x;
            const cplx alpha = cdiv(rho, sg);
            int code = ST_OK;
            if (!fin(sg) || (sg.x == 0.0 && sg.y == 0.0)) code = ST_SIGMA;
            else if (!fin(alpha)) code = ST_ALPHA;
            skip = (st != 0.0) || code != ST_OK; as = alpha;
            if (blockIdx.x == 0) {
                scal[S_SIGMA] = sg; scal[S_ALPHA] = alpha;
                if (st == 0.0 && code != ST_OK) scal[S_STATUS] = make_double2((double)code, (double)cycle);
            }
        }
    }
    __syncthreads();
    if (skip) return;
    const cplx alpha = as;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        cplx u[NV + 1], r[NV];
#pragma unroll
        for (int k = 0; k <= NV; ++k) u[k] = us[(int64_t)k * ld + i];
#pragma unroll
        for (int k = 0; k < NV; ++k) r[k] = rs[(int64_t)k * ld + i];
        x[i] = caddmul(x[i], alpha, u[0]);
#pragma unroll
        for (int k = 0; k < NV; ++k) rs[(int64_t)k * ld + i] = csubmul(r[k], alpha, u[k + 1]);
    }
}

// partial[(P_GRAM + e) * RED_BLOCKS + block] = slice of <rs[a], rs[b]>, e = packed index of a <= b < NV (row after row)
template <int NV>
__global__ __launch_bounds__(RED_THREADS) void k_gram(Members B) {
    __shared__ cplx sh[RED_THREADS / 64];
    const int m = B.m[blockIdx.y];
    const int64_t n = B.n, ld = B.n;
    const cplx* __restrict__ rs = m_work(B, m);
    cplx* __restrict__ partial = m_partial(B, m);
    constexpr int NE = NV * (NV + 1) / 2;
    cplx acc[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) acc[e] = make_double2(0.0, 0.0);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        cplx v[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] = rs[(int64_t)k * ld + i];
        int e = 0;
#pragma unroll
        for (int a = 0; a < NV; ++a) {
            cnorm_acc(acc[e], v[a]);                                            // the diagonal is real
            ++e;
#pragma unroll
            for (int b = a + 1; b < NV; ++b, ++e) cdot_acc(acc[e], v[a], v[b]);
        }
    }
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const cplx r = block_sum(acc[e], sh);
        if (threadIdx.x == 0) partial[(int64_t)(P_GRAM + e) * RED_BLOCKS + blockIdx.x] = r;
        __syncthreads();
    }
}

// One wave per member.  G from the partials (published in scal[S_G..], row-major NVMAX x NVMAX); G[0,0] <= tol^2: the
// Krylov space is exhausted, status ST_EXHAUSTED and no solve of a singular G.  Otherwise gamma = G[1:,1:] \ G[1:,0] by LU
// with partial pivoting (largest |.|^2 of the column, the lowest row on a tie) and sigma = -(sigma gamma_{l-1}): the
// factor of the MR part and the sign flip that opens the next cycle.
template <bool TEAM>
__global__ __launch_bounds__(64) void k_mr_solve(Members B, int nb, int nv, int cycle) {
    __shared__ cplx G[NVMAX][NVMAX];
    const int m = B.m[blockIdx.y];
    cplx* scal = m_scal(B, m);
    int e = 0;
    for (int a = 0; a < nv; ++a)
        for (int b = a; b < nv; ++b, ++e) {
            const cplx g = slot_sum<TEAM>(B, m, P_GRAM + e, nb);
            if (threadIdx.x == 0) { G[a][b] = g; G[b][a] = make_double2(g.x, -g.y); }
        }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int a = 0; a < nv; ++a) for (int b = 0; b < nv; ++b) scal[S_G + a * NVMAX + b] = G[a][b];
    if (scal[S_STATUS].x != 0.0) return;
    if (G[0][0].x <= B.tol2[m]) { scal[S_STATUS] = make_double2((double)ST_EXHAUSTED, (double)cycle); return; }
    const int l = nv - 1;
    cplx M[LMAX][LMAX], y[LMAX];
    for (int a = 0; a < l; ++a) { y[a] = G[a + 1][0]; for (int b = 0; b < l; ++b) M[a][b] = G[a + 1][b + 1]; }
    bool ok = true;
    for (int p = 0; p < l && ok; ++p) {
        int piv = p; double best = fma(M[p][p].x, M[p][p].x, M[p][p].y * M[p][p].y);
        for (int a = p + 1; a < l; ++a) { const double m2 = fma(M[a][p].x, M[a][p].x, M[a][p].y * M[a][p].y); if (m2 > best) { best = m2; piv = a; } }
        if (!(best > 0.0) || !isfinite(best)) { ok = false; break; }
        if (piv != p) { for (int b = 0; b < l; ++b) { const cplx t = M[p][b]; M[p][b] = M[piv][b]; M[piv][b] = t; } const cplx t = y[p]; y[p] = y[piv]; y[piv] = t; }
        for (int a = p + 1; a < l; ++a) {
            const cplx f = cdiv(M[a][p], M[p][p]);
            for (int b = p + 1; b < l; ++b) M[a][b] = csubmul(M[a][b], f, M[p][b]);
            y[a] = csubmul(y[a], f, y[p]);
        }
    }
    if (ok) {
        for (int a = l - 1; a >= 0; --a) {
            cplx acc = y[a];
            for (int b = a + 1; b < l; ++b) acc = csubmul(acc, M[a][b], y[b]);
            y[a] = cdiv(acc, M[a][a]);
            ok = ok && fin(y[a]);
        }
    }
    if (!ok) { scal[S_STATUS] = make_double2((double)ST_GAMMA, (double)cycle); return; }
    for (int a = 0; a < l; ++a) scal[S_GAMMA + a] = y[a];
    const cplx s = cmul(scal[S_SIGMA], y[l - 1]);
    scal[S_SIGMA] = make_double2(-s.x, -s.y);
}

// us[0] -= sum gamma_i us[i+1]; x += sum gamma_i rs[i]; rs[0] -= sum gamma_i rs[i+1] (i < L); partial slot P_NORM: |rs[0]|^2
template <int L>
__global__ __launch_bounds__(RED_THREADS) void k_mr_update(Members B, int64_t uoff) {
    __shared__ cplx sh[RED_THREADS / 64];
    __shared__ cplx gs[L];
    const int m = B.m[blockIdx.y];
    const int64_t n = B.n, ld = B.n;
    cplx* __restrict__ rs = m_work(B, m);
    cplx* __restrict__ us = m_work(B, m) + uoff;
    cplx* __restrict__ x = B.x + (int64_t)m * n;
    const cplx* __restrict__ scal = m_scal(B, m);
    if (scal[S_STATUS].x != 0.0) return;                 // (written by the kernels before this one only)
    if (threadIdx.x < L) gs[threadIdx.x] = scal[S_GAMMA + threadIdx.x];
    __syncthreads();
    cplx g[L];
#pragma unroll
    for (int k = 0; k < L; ++k) g[k] = gs[k];
    cplx nrm = make_double2(0.0, 0.0);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        cplx u[L + 1], r[L + 1];
#pragma unroll
        for (int k = 0; k <= L; ++k) { u[k] = us[(int64_t)k * ld + i]; r[k] = rs[(int64_t)k * ld + i]; }
        cplx xv = x[i], u0 = u[0], r0 = r[0];
#pragma unroll
        for (int k = 0; k < L; ++k) {
            u0 = csubmul(u0, g[k], u[k + 1]);
            xv = caddmul(xv, g[k], r[k]);
            r0 = csubmul(r0, g[k], r[k + 1]);
        }
        us[i] = u0; x[i] = xv; rs[i] = r0;
        cnorm_acc(nrm, r0);
    }
    const cplx s = block_sum(nrm, sh);
    if (threadIdx.x == 0) m_partial(B, m)[(int64_t)P_NORM * RED_BLOCKS + blockIdx.x] = s;
}

// scal[S_RES] = sqrt(sum of the P_NORM partials), unless the cycle ended without an MR update
template <bool TEAM>
__global__ __launch_bounds__(64) void k_res_finish(Members B, int nb) {
    const int m = B.m[blockIdx.y];
    cplx* scal = m_scal(B, m);
    const cplx s = slot_sum<TEAM>(B, m, P_NORM, nb);
    if (threadIdx.x == 0 && scal[S_STATUS].x == 0.0) scal[S_RES] = make_double2(sqrt(s.x), 0.0);
}

struct Pinned {
    cplx* p = nullptr;
    void alloc(size_t count) { LSFC_HIP(hipHostMalloc((void**)&p, count * sizeof(cplx))); }
    ~Pinned() { if (p) (void)hipHostFree(p); }
};
struct Event {
    hipEvent_t e = nullptr;
    void create() { LSFC_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming)); }
    ~Event() { if (e) (void)hipEventDestroy(e); }
};

// what the host keeps per member
struct Solve {
    double tol = 0.0, current = 0.0;
    bool converged = false;
    int bad = ST_OK, bad_cycle = 0;
    int64_t cycles = 0, mvps = 0;
};

// What the solve keeps per slab of the team (team.hpp: the plan itself with all nrhs members, n = N, or rank `rank` of a
// multi-device plan with its z slab of the one member): what the kernels of that device work on.
struct Rank : RankSlab {
    cplx* x = nullptr; const cplx* b = nullptr;
    DevBuf<cplx> work, scal, partial, table;
    DevBuf<double> tol2;
    Event ready, consumed;                  // TEAM: my rank sums have reached every table / my kernels so far have read my table
    Members B{};                            // of this rank's launches; B.m: the member list of the round
    Rank(const RankSlab& s, cplx* x_, const cplx* b_) : RankSlab(s), x(x_), b(b_) {}
};
using Ranks = std::vector<std::unique_ptr<Rank>>;

} // namespace

// nrhs solves in lock step over the ranks: one (the plan; TEAM = false) or the P ranks of a multi-device plan (TEAM, nrhs = 1,
// the form of k_rank_sum), every step enqueued rank by rank from the calling thread.  Per rank: x (in/out) and b, nrhs
// device vectors of n back to back.  r_shadow (may be NULL): nrhs vectors of N complex on the device, or on the host
// (shadow_on_host; TEAM: always, the whole vector); resnorm: nrhs rows of cap entries.  pc takes the active members of every
// round (Precond::apply; TEAM: a host callback on the whole vector, gathered from the slabs and scattered back).
// code[2 j], code[2 j + 1]: LSFC_BICG_* of member j and its cycle (of the breakdown, else the last one).
template <bool TEAM>
static void bicgstabl_run_as(const SlabTeam& T, Ranks& ranks, int nrhs, const cplx* r_shadow, bool shadow_on_host, const Precond& pc,
                          const lsfc_bicgstabl_opts& o, int l, int64_t maxmv, double reltol, double abstol, double* resnorm, int64_t cap,
                          lsfc_gmres_result* res, int64_t* code) {
    const int P = (int)ranks.size(), nv = l + 1;
    Rank& k0 = *ranks[0];
    lsfc_plan* root = T.root;
    const int64_t N = root->N, n = k0.n;                // (the slabs of a multi-device plan are equal)
    const int nb = blas_red_blocks(n);
    const int64_t wstride = (int64_t)(2 * l + 3) * n, uoff = (int64_t)nv * n, toff = 2 * (int64_t)nv * n;
    // (TEAM = false: one slab, whose device is current -- no call of the runtime around f)
    auto each = [&](auto&& f) { if constexpr (TEAM) T.each([&](const RankSlab& s) { f(*ranks[(size_t)s.rank]); }); else f(k0); };
    each([&](Rank& k) {
        k.work.alloc((size_t)nrhs * (size_t)wstride);
        k.scal.alloc((size_t)nrhs * S_COUNT);
        k.partial.alloc((size_t)nrhs * P_SLOTS * RED_BLOCKS);
        k.tol2.alloc((size_t)nrhs);
        k.B.work = k.work.p; k.B.x = k.x; k.B.scal = k.scal.p; k.B.partial = k.partial.p; k.B.tol2 = k.tol2.p; k.B.wstride = wstride; k.B.n = n;
        k.B.rank = k.rank; k.B.nranks = P;
        if constexpr (TEAM) {
            k.table.alloc((size_t)P * P_SLOTS);
            LSFC_HIP(hipMemsetAsync(k.table.p, 0, k.table.bytes(), k.st()));
            k.B.table = k.table.p;
            k.ready.create(); k.consumed.create();
        }
    });
    auto R = [&](Rank& k, int m, int i) { return k.work.p + (size_t)m * (size_t)wstride + (size_t)i * (size_t)n; };
    auto U = [&](Rank& k, int m, int i) { return R(k, m, nv + i); };
    if constexpr (TEAM) LSFC_HIP(hipSetDevice(k0.device));
    // hs: the scalar blocks as fetched; TEAM: a second block, the initial scalars that every rank uploads (rank 0's fetch must not land on them)
    Pinned hs, ht, vpin; hs.alloc((size_t)(TEAM ? 2 : 1) * (size_t)nrhs * S_COUNT); ht.alloc((size_t)(nrhs + 1) / 2);
    cplx* const hinit = hs.p + (TEAM ? (size_t)nrhs * S_COUNT : 0);
    if (pc.fn && !pc.on_device) vpin.alloc((size_t)N);
    Event fetched; fetched.create();
    // the member list of the launches that follow
    auto select = [&](const std::vector<int>& list) { each([&](Rank& k) { for (size_t a = 0; a < list.size(); ++a) k.B.m[a] = list[a]; }); };

    // the operator on vector `in(k, m)` of every member of the list, in groups that share one pass of the pipeline
    std::vector<const cplx*> av;
    std::vector<cplx*> pv;
    auto apply = [&](const std::vector<int>& list, auto&& in, auto&& out) {
        av.clear(); pv.clear();
        if constexpr (TEAM) {
            for (auto& k : ranks) { av.push_back(in(*k, 0)); pv.push_back(out(*k, 0)); }
            T.apply(av.data(), pv.data());
        } else {
            for (int m : list) { av.push_back(in(k0, m)); pv.push_back(out(k0, m)); }
            plan_apply_batch_dev(root, av.data(), pv.data(), list.size());
        }
    };
    auto precondition = [&](const std::vector<int>& list, auto&& v) {
        if constexpr (TEAM) {
            if (pc.fn) T.host_precond(pc, vpin.p, [&](const RankSlab& s) { return v(*ranks[(size_t)s.rank], 0); });
        } else {
            pv.clear();
            for (int m : list) pv.push_back(v(k0, m));
            pc.apply(pv.data(), pv.size(), vpin.p, k0.st());
        }
    };
    // TEAM: completes the partial slots [slot0, slot0 + cnt) across the ranks, between the kernels that wrote the partials and
    // the one that consumes the sums.  Ordered by events alone, both ways: a rank's copies wait until every other rank has got
    // past the kernels that read the entries they replace (consumed), the consumer waits for the copies of all ranks (ready).
    auto reduce = [&](int slot0, int cnt) {
        if constexpr (TEAM) {
            each([&](Rank& k) { LSFC_HIP(hipEventRecord(k.consumed.e, k.st())); });
            each([&](Rank& k) {
                hipLaunchKernelGGL(k_rank_sum, dim3((unsigned)cnt), dim3(64), 0, k.st(), k.B, slot0, nb);
                const size_t row = (size_t)k.rank * P_SLOTS + (size_t)slot0, bytes = (size_t)cnt * sizeof(cplx);
                for (int s = 1; s < P; ++s) {               // every source starts with a different peer
                    Rank& q = *ranks[(size_t)((k.rank + s) % P)];
                    LSFC_HIP(hipStreamWaitEvent(k.st(), q.consumed.e, 0));
                    if (q.device == k.device) LSFC_HIP(hipMemcpyAsync(q.table.p + row, k.table.p + row, bytes, hipMemcpyDeviceToDevice, k.st()));
                    else LSFC_HIP(hipMemcpyPeerAsync(q.table.p + row, q.device, k.table.p + row, k.device, bytes, k.st()));
                }
                LSFC_HIP(hipEventRecord(k.ready.e, k.st()));
            });
            each([&](Rank& k) { for (auto& q : ranks) if (q->rank != k.rank) LSFC_HIP(hipStreamWaitEvent(k.st(), q->ready.e, 0)); });
        } else { (void)slot0; (void)cnt; }
    };
    // all members' scalars in one copy (the ranks' scalar blocks agree: rank 0's)
    auto fetch = [&]() {
        if constexpr (TEAM) LSFC_HIP(hipSetDevice(k0.device));
        LSFC_HIP(hipMemcpyAsync(hs.p, k0.scal.p, (size_t)nrhs * S_COUNT * sizeof(cplx), hipMemcpyDeviceToHost, k0.st()));
        LSFC_HIP(hipEventRecord(fetched.e, k0.st()));
        LSFC_HIP(hipEventSynchronize(fetched.e));
    };
    auto H = [&](int m) { return hs.p + (size_t)m * S_COUNT; };
    // scal[S_RES] = ||rs[0]|| of the members of the list
    auto norm0 = [&](const std::vector<int>& list) {
        select(list);
        each([&](Rank& k) { hipLaunchKernelGGL(k_dot, dim3(nb, (unsigned)list.size()), dim3(RED_THREADS), 0, k.st(), k.B, (int64_t)0, (int64_t)0, (int)P_NORM); });
        reduce(P_NORM, 1);
        each([&](Rank& k) { hipLaunchKernelGGL(k_norm_finish<TEAM>, dim3(1, (unsigned)list.size()), dim3(64), 0, k.st(), k.B, nb); });
    };

    // init: rs[0] = Pl \ (b - A x), us = 0, shadow residual, sigma = -1 (sigma = 1, negated by the first cycle)
    std::vector<Solve> S((size_t)nrhs);
    std::vector<int> act((size_t)nrhs);
    for (int m = 0; m < nrhs; ++m) act[(size_t)m] = m;
    select(act);
    if (o.initially_zero) {
        each([&](Rank& k) {
            for (int m = 0; m < nrhs; ++m) LSFC_HIP(hipMemcpyAsync(R(k, m, 0), k.b + (size_t)m * n, (size_t)n * sizeof(cplx), hipMemcpyDeviceToDevice, k.st()));
        });
    } else {
        apply(act, [&](Rank& k, int m) { return (const cplx*)(k.x + (size_t)m * n); }, [&](Rank& k, int m) { return R(k, m, 0); });
        each([&](Rank& k) { hipLaunchKernelGGL(k_residual, dim3(grid_for(n), (unsigned)nrhs), dim3(256), 0, k.st(), k.B, k.b); });
        for (auto& s : S) s.mvps = 1;
    }
    precondition(act, [&](Rank& k, int m) { return R(k, m, 0); });
    for (size_t i = 0; i < (size_t)nrhs * S_COUNT; ++i) hinit[i] = make_double2(0.0, 0.0);
    for (int m = 0; m < nrhs; ++m) hinit[(size_t)m * S_COUNT + S_SIGMA] = make_double2(-1.0, 0.0);
    each([&](Rank& k) {
        for (int m = 0; m < nrhs; ++m) {
            LSFC_HIP(hipMemsetAsync(U(k, m, 0), 0, (size_t)nv * (size_t)n * sizeof(cplx), k.st()));
            const cplx* sh = r_shadow ? r_shadow + (size_t)m * N + k.off : R(k, m, 0);
            LSFC_HIP(hipMemcpyAsync(R(k, m, 2 * nv), sh, (size_t)n * sizeof(cplx), r_shadow && shadow_on_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, k.st()));
        }
        LSFC_HIP(hipMemcpyAsync(k.scal.p, hinit, (size_t)nrhs * S_COUNT * sizeof(cplx), hipMemcpyHostToDevice, k.st()));
    });
    norm0(act);
    LSFC_HIP(hipGetLastError());
    fetch();
    double* t2 = (double*)ht.p;
    for (int m = 0; m < nrhs; ++m) {
        Solve& s = S[(size_t)m];
        const double beta0 = H(m)[S_RES].x;
        s.tol = std::max(reltol * beta0, abstol);
        s.current = beta0;
        s.converged = beta0 <= s.tol;
        s.bad = std::isfinite(beta0) ? ST_OK : ST_RESIDUAL;
        t2[m] = s.tol * s.tol;
    }
    each([&](Rank& k) { LSFC_HIP(hipMemcpyAsync(k.tol2.p, t2, (size_t)nrhs * sizeof(double), hipMemcpyHostToDevice, k.st())); });
    auto running = [&](const Solve& s) { return !s.converged && s.bad == ST_OK && s.mvps < maxmv; };
    auto still_active = [&]() { std::vector<int> a; for (int m = 0; m < nrhs; ++m) if (running(S[(size_t)m])) a.push_back(m); return a; };
    act = still_active();
    std::vector<int> broke;

    // every member of the list is in the same cycle: all start at 0 and a member never rejoins
    for (int64_t cycles = 0; !act.empty(); ++cycles) {
        const int cyc = (int)std::min<int64_t>(cycles + 1, 1 << 30);
        select(act);
        const dim3 grid((unsigned)nb, (unsigned)act.size()), one(1, (unsigned)act.size());
        for (int j = 0; j < l; ++j) {                       // BiCG part
            each([&](Rank& k) { hipLaunchKernelGGL(k_dot, grid, dim3(RED_THREADS), 0, k.st(), k.B, toff, (int64_t)j * n, (int)P_RHO); });
            reduce(P_RHO, 1);
            dispatch<1, LMAX>(j + 1, "bicgstabl", [&](auto nvj) {
                each([&](Rank& k) { hipLaunchKernelGGL((k_bicg_u<decltype(nvj)::value, TEAM>), grid, dim3(RED_THREADS), 0, k.st(), k.B, uoff, nb, cyc); });
            });
            apply(act, [&](Rank& k, int m) { return (const cplx*)U(k, m, j); }, [&](Rank& k, int m) { return U(k, m, j + 1); });
            precondition(act, [&](Rank& k, int m) { return U(k, m, j + 1); });
            each([&](Rank& k) { hipLaunchKernelGGL(k_dot, grid, dim3(RED_THREADS), 0, k.st(), k.B, toff, uoff + (int64_t)(j + 1) * n, (int)P_SIGMA); });
            reduce(P_SIGMA, 1);
            dispatch<1, LMAX>(j + 1, "bicgstabl", [&](auto nvj) {
                each([&](Rank& k) { hipLaunchKernelGGL((k_bicg_rx<decltype(nvj)::value, TEAM>), grid, dim3(RED_THREADS), 0, k.st(), k.B, uoff, nb, cyc); });
            });
            apply(act, [&](Rank& k, int m) { return (const cplx*)R(k, m, j); }, [&](Rank& k, int m) { return R(k, m, j + 1); });
            precondition(act, [&](Rank& k, int m) { return R(k, m, j + 1); });
        }
        dispatch<2, NVMAX>(nv, "bicgstabl", [&](auto nvc) {              // MR part
            each([&](Rank& k) { hipLaunchKernelGGL((k_gram<decltype(nvc)::value>), grid, dim3(RED_THREADS), 0, k.st(), k.B); });
        });
        reduce(P_GRAM, nv * (nv + 1) / 2);
        each([&](Rank& k) { hipLaunchKernelGGL(k_mr_solve<TEAM>, one, dim3(64), 0, k.st(), k.B, nb, nv, cyc); });
        dispatch<1, LMAX>(l, "bicgstabl", [&](auto lc) {
            each([&](Rank& k) { hipLaunchKernelGGL((k_mr_update<decltype(lc)::value>), grid, dim3(RED_THREADS), 0, k.st(), k.B, uoff); });
        });
        reduce(P_NORM, 1);
        each([&](Rank& k) { hipLaunchKernelGGL(k_res_finish<TEAM>, one, dim3(64), 0, k.st(), k.B, nb); });
        LSFC_HIP(hipGetLastError());
        fetch();
        broke.clear();
        for (int m : act) {
            Solve& s = S[(size_t)m];
            s.mvps += 2 * l;
            const int status = (int)H(m)[S_STATUS].x;
            if (status == ST_OK) {
                s.current = H(m)[S_RES].x;
                if (!std::isfinite(s.current)) { s.bad = ST_RESIDUAL; s.bad_cycle = cyc; }
            } else if (status == ST_EXHAUSTED) {
                s.current = std::sqrt(H(m)[S_G].x);
                s.converged = true;
            } else {
                // breakdown: x and rs[0] are the last finite pair -- the residual of that iterate decides (a breakdown with
                // the residual already below the tolerance is the exhausted Krylov space met one step early)
                s.bad = status; s.bad_cycle = (int)H(m)[S_STATUS].y;
                broke.push_back(m);
            }
        }
        if (!broke.empty()) {
            norm0(broke);
            LSFC_HIP(hipGetLastError());
            fetch();
            for (int m : broke) S[(size_t)m].current = H(m)[S_RES].x;
        }
        for (int m : act) {
            Solve& s = S[(size_t)m];
            if (resnorm && s.cycles < cap) resnorm[(size_t)m * (size_t)cap + (size_t)s.cycles] = s.current;
            ++s.cycles;
            s.converged = s.converged || s.current <= s.tol;
        }
        act = still_active();
    }
    each([&](Rank& k) { LSFC_HIP(hipStreamSynchronize(k.st())); });
    for (int m = 0; m < nrhs; ++m) {
        const Solve& s = S[(size_t)m];
        res[m].iters = s.cycles; res[m].mvps = s.mvps; res[m].converged = s.converged ? 1 : 0; res[m].final_resnorm = s.current;
        code[2 * m] = s.converged ? LSFC_BICG_CONVERGED : (s.bad != ST_OK ? s.bad : LSFC_BICG_MAX_MV);
        code[2 * m + 1] = (!s.converged && s.bad != ST_OK) ? s.bad_cycle : s.cycles;
    }
}

// the form of the solve follows the plan: the team form on a multi-device plan (whatever its number of ranks)
static void bicgstabl_run(const SlabTeam& T, Ranks& ranks, int nrhs, const cplx* r_shadow, bool shadow_on_host, const Precond& pc,
                          const lsfc_bicgstabl_opts& o, int l, int64_t maxmv, double reltol, double abstol, double* resnorm, int64_t cap,
                          lsfc_gmres_result* res, int64_t* code) {
    if (T.multi) bicgstabl_run_as<true>(T, ranks, nrhs, r_shadow, shadow_on_host, pc, o, l, maxmv, reltol, abstol, resnorm, cap, res, code);
    else bicgstabl_run_as<false>(T, ranks, nrhs, r_shadow, shadow_on_host, pc, o, l, maxmv, reltol, abstol, resnorm, cap, res, code);
}

// The memory rule of a solve on a multi-device plan, per DEVICE, before its host vectors are staged: every rank on it needs 2 l + 3
// work vectors of N / P complex, and its staged x and b where its staging buffers do not hold them yet.
static void team_stage(const SlabTeam& T, int l) {
    for (const RankSlab& s : T.slabs) {
        int first = s.rank, on = 0; double need = 0.0;
        for (const RankSlab& q : T.slabs) if (q.device == s.device) {
            first = std::min(first, q.rank); ++on;
            need += ((double)(2 * l + 3) + (q.p->xs.n < (size_t)q.n ? 2.0 : 0.0)) * (double)q.n * sizeof(cplx);
        }
        if (first != s.rank) continue;                  // (a device is checked once, at its first rank)
        size_t free_b = 0, total_b = 0;
        LSFC_HIP(hipSetDevice(s.device));
        LSFC_HIP(hipMemGetInfo(&free_b, &total_b));
        if (need > (double)free_b)
            fail(LSFC_ENOMEM, "lsfc_bicgstabl_multi: device %d: %d rank%s x (2 l + 3 = %d work vectors, + staged x and b) of %lld complex need %.1f GB of "
                 "device memory, %.1f GB are free there -- lower l or spread the plan over more devices", s.device, on, on == 1 ? "" : "s", 2 * l + 3,
                 (long long)s.n, need / 1e9, (double)free_b / 1e9);
    }
}

// the argument checks of the entry points, before any device call.  team: lsfc_bicgstabl_multi, the entry point of multi-device plans --
// lsfc_bicgstabl and lsfc_bicgstabl_batch refuse them as they always have, so what a caller of those sees does not change
static void check_args(const char* fn, bool batch, bool team, lsfc_plan* plan, const double* x, const double* b, const lsfc_bicgstabl_opts* opts,
                       const double* resnorm, int64_t resnorm_cap, const lsfc_gmres_result* result, int memspace) {
    LSFC_REQUIRE(opts, "%s: NULL opts", fn);
    LSFC_REQUIRE(opts->l >= 1 && opts->l <= LMAX, "%s: l = %d is outside 1..%d", fn, opts->l, LMAX);
    for (int i = 0; i < 4; ++i) LSFC_REQUIRE(opts->reserved[i] == 0, "%s: reserved[%d] is not zero", fn, i);
    LSFC_REQUIRE(memspace == LSFC_MEM_HOST || memspace == LSFC_MEM_DEVICE, "%s: unknown memspace %d", fn, memspace);
    LSFC_REQUIRE(plan && x && b && result, "%s: NULL argument", fn);
    LSFC_REQUIRE(resnorm || resnorm_cap <= 0, "%s: NULL resnorm with a capacity of %lld", fn, (long long)resnorm_cap);
    if (!team) {
        LSFC_REQUIRE(!plan->multi && !plan->dist, "%s runs on a single-device plan (not a distributed or multi-device one)%s", fn,
                     batch ? ": batched BiCGStab(l) is not offered there" : "; lsfc_bicgstabl_multi solves on a single-process multi-device plan");
        return;
    }
    LSFC_REQUIRE(plan->multi, "%s runs on a single-process multi-device plan (lsfc_plan_create_gv3d_multi): %s", fn,
                 plan->dist ? "a multi-process distributed plan (lsfc_dist_plan_create_gv3d) is not offered" : "lsfc_bicgstabl solves on a single-device plan");
    LSFC_REQUIRE(memspace == LSFC_MEM_HOST, "%s: a multi-device plan takes host vectors (LSFC_MEM_DEVICE is not offered there)", fn);
    LSFC_REQUIRE(!(opts->precond && opts->precond_on_device), "%s: a multi-device plan takes a host preconditioner callback "
                 "(precond_on_device = 1 is not offered there)", fn);
}

} // namespace lsfc

using namespace lsfc;

// Both entry points (defined below them): the argument checks, the option defaults, the memory rule (nrhs (2 l + 3) work vectors; host vectors:
// the staged x and b, 2 nrhs vectors, on top -- r_shadow is uploaded into its work vector), host staging through
// plan->xs / plan->ys, and the solve.  A multi-device plan (lsfc_bicgstabl_multi): the same per rank and slab, the memory rule per device.  batch: the texts of lsfc_bicgstabl_batch, and its members meet at the library's
// own preconditioner; the single call has nobody to meet there and calls the callback as given.
static void bicgstabl_entry(const char* fn, bool batch, bool team, lsfc_plan* plan, double* x, const double* b, int64_t nrhs, const lsfc_bicgstabl_opts* opts,
                            double* resnorm, int64_t resnorm_cap, lsfc_gmres_result* results, int64_t* code, int memspace);

// one solve: lsfc_bicgstabl, or (team) lsfc_bicgstabl_multi
static int bicgstabl_single(const char* fn, bool team, lsfc_plan* plan, double* x, const double* b, const lsfc_bicgstabl_opts* opts, double* resnorm,
                            int64_t resnorm_cap, lsfc_gmres_result* result, int memspace) {
    int64_t code[2] = { 0, 0 };
    const int rc = guarded([&] { bicgstabl_entry(fn, false, team, plan, x, b, 1, opts, resnorm, resnorm_cap, result, code, memspace); });
    if (rc != LSFC_OK || result->converged) return rc;
    if (code[0] != LSFC_BICG_MAX_MV) set_last_error("bicgstabl: breakdown in cycle %d: %s; x is the last finite iterate", (int)code[1], ST_NAME[code[0]]);
    else set_last_error("bicgstabl: max_mv_products reached without convergence");
    return LSFC_ENOTCONV;
}

extern "C" int lsfc_bicgstabl(lsfc_plan* plan, double* x, const double* b, const lsfc_bicgstabl_opts* opts, double* resnorm,
                              int64_t resnorm_cap, lsfc_gmres_result* result, int memspace) {
    return bicgstabl_single("lsfc_bicgstabl", false, plan, x, b, opts, resnorm, resnorm_cap, result, memspace);
}

extern "C" int lsfc_bicgstabl_multi(lsfc_plan* plan, double* x, const double* b, const lsfc_bicgstabl_opts* opts, double* resnorm,
                                    int64_t resnorm_cap, lsfc_gmres_result* result, int memspace) {
    return bicgstabl_single("lsfc_bicgstabl_multi", true, plan, x, b, opts, resnorm, resnorm_cap, result, memspace);
}

extern "C" int lsfc_bicgstabl_batch(lsfc_plan* plan, double* x, const double* b, int64_t nrhs, const lsfc_bicgstabl_opts* opts, double* resnorm,
                                    int64_t resnorm_cap, lsfc_gmres_result* results, int64_t* status, int memspace) {
    int64_t code[2 * KRYLOV_NRHS_MAX] = { 0 };
    const int rc = guarded([&] {
        bicgstabl_entry("lsfc_bicgstabl_batch", true, false, plan, x, b, nrhs, opts, resnorm, resnorm_cap, results, code, memspace);
        if (status) for (int64_t i = 0; i < 2 * nrhs; ++i) status[i] = code[i];
    });
    if (rc != LSFC_OK) return rc;
    // LSFC_OK whatever the members did (the rule of lsfc_gmres_batch); the message names the first that did not converge
    for (int64_t j = 0; j < nrhs; ++j) {
        const int64_t c = code[(size_t)(2 * j)], cyc = code[(size_t)(2 * j + 1)];
        if (c == LSFC_BICG_CONVERGED) continue;
        if (c == LSFC_BICG_MAX_MV) set_last_error("bicgstabl_batch: right-hand side %lld: max_mv_products reached without convergence in cycle %lld", (long long)j, (long long)cyc);
        else set_last_error("bicgstabl_batch: right-hand side %lld: breakdown in cycle %lld: %s; its x is the last finite iterate", (long long)j, (long long)cyc, ST_NAME[c]);
        break;
    }
    return LSFC_OK;
}

static void bicgstabl_entry(const char* fn, bool batch, bool team, lsfc_plan* plan, double* x, const double* b, int64_t nrhs, const lsfc_bicgstabl_opts* opts,
                            double* resnorm, int64_t resnorm_cap, lsfc_gmres_result* results, int64_t* code, int memspace) {
    if (batch) LSFC_REQUIRE(nrhs >= 1 && nrhs <= KRYLOV_NRHS_MAX, "%s: nrhs = %lld is outside 1..%d", fn, (long long)nrhs, KRYLOV_NRHS_MAX);
    check_args(fn, batch, team, plan, x, b, opts, resnorm, resnorm_cap, results, memspace);
    const int l = opts->l, n = (int)nrhs;
    const int64_t N = plan->N;
    const int64_t maxmv = opts->max_mv_products > 0 ? opts->max_mv_products : N;
    const double reltol = opts->reltol >= 0 ? opts->reltol : DEFAULT_RELTOL;
    const double abstol = opts->abstol > 0 ? opts->abstol : 0.0;
    const int64_t cap = resnorm_cap > 0 ? resnorm_cap : 0;
    plan_check_precond_op(plan, opts->precond, opts->precond_user, fn);
    const Precond pc(opts->precond, opts->precond_user, opts->precond_on_device != 0, batch, N, fn);
    const SlabTeam T(plan);
    Ranks ranks;
    const bool multi = T.multi, host = memspace == LSFC_MEM_HOST;
    const size_t bytes = (size_t)n * (size_t)N * sizeof(cplx);
    if (multi) {
        team_stage(T, l);
        T.scatter((const cplx*)x, (const cplx*)b);
        for (const RankSlab& s : T.slabs) ranks.emplace_back(new Rank(s, s.p->xs.p, s.p->ys.p));
    } else {
        LSFC_HIP(hipSetDevice(plan->device));
        const bool stage = host && plan->xs.n < (size_t)n * (size_t)N;
        size_t free_b = 0, total_b = 0;
        LSFC_HIP(hipMemGetInfo(&free_b, &total_b));
        const double per = ((double)(2 * l + 3) + (stage ? 2.0 : 0.0)) * (double)N * sizeof(cplx);
        if ((double)n * per > (double)free_b) {
            if (!batch)
                fail(LSFC_ENOMEM, "lsfc_bicgstabl: (2 l + 3 = %d work vectors%s) of %lld complex need %.1f GB of device memory, %.1f GB are free "
                     "-- lower l", 2 * l + 3, stage ? " + staged x and b" : "", (long long)N, per / 1e9, (double)free_b / 1e9);
            fail(LSFC_ENOMEM, "lsfc_bicgstabl_batch: %d right-hand sides x (2 l + 3 = %d work vectors%s) of %lld complex need %.1f GB of device memory, "
                 "%.1f GB are free -- %lld right-hand sides would fit; solve fewer per call or lower l", n, 2 * l + 3, stage ? " + staged x and b" : "",
                 (long long)N, (double)n * per / 1e9, (double)free_b / 1e9, (long long)((double)free_b / per));
        }
        const cplx* xd = (const cplx*)x; const cplx* bd = (const cplx*)b;
        if (host) {
            if (stage) { plan->xs.alloc((size_t)n * (size_t)N); plan->ys.alloc((size_t)n * (size_t)N); }     // (plan_ensure_staging, with the `stage` the memory rule counted)
            LSFC_HIP(hipMemcpy(plan->xs.p, x, bytes, hipMemcpyHostToDevice));
            LSFC_HIP(hipMemcpy(plan->ys.p, b, bytes, hipMemcpyHostToDevice));
            xd = plan->xs.p; bd = plan->ys.p;
        }
        ranks.emplace_back(new Rank(T.slabs[0], (cplx*)xd, bd));
    }
    bicgstabl_run(T, ranks, n, (const cplx*)opts->r_shadow, host, pc, *opts, l, maxmv, reltol, abstol, resnorm, cap, results, code);
    if (multi) { T.gather((cplx*)x); T.sync(); LSFC_HIP(hipSetDevice(plan->device)); }
    else if (host) LSFC_HIP(hipMemcpy(x, plan->xs.p, bytes, hipMemcpyDeviceToHost));
}
