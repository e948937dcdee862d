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
#include "plan.hpp"
#include "krylov_blas.hpp"
#include "reduce.hpp"
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
    int64_t wstride, n;
    int m[KRYLOV_NRHS_MAX];
};
__device__ __forceinline__ cplx* m_work(const Members& B, int m) { return B.work + (int64_t)m * B.wstride; }
__device__ __forceinline__ cplx* m_scal(const Members& B, int m) { return B.scal + (int64_t)m * S_COUNT; }
__device__ __forceinline__ cplx* m_partial(const Members& B, int m) { return B.partial + (int64_t)m * (P_SLOTS * RED_BLOCKS); }

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
__global__ __launch_bounds__(64) void k_norm_finish(Members B, int nb) {
    const int m = B.m[blockIdx.y];
    const cplx s = finish_in_wave(m_partial(B, m) + (int64_t)P_NORM * RED_BLOCKS, nb);
    if (threadIdx.x == 0) m_scal(B, m)[S_RES] = make_double2(sqrt(s.x), 0.0);
}

// rho = sum of the P_RHO partials, beta = rho / sigma; us[i] = rs[i] - beta us[i] for i < NV (= j + 1); block 0 publishes rho, beta
template <int NV>
__global__ __launch_bounds__(RED_THREADS) void k_bicg_u(Members B, int64_t uoff, int nb, int cycle) {
    __shared__ cplx bs; __shared__ int skip;
    const int m = B.m[blockIdx.y];
    const int64_t n = B.n, ld = B.n;
    const cplx* __restrict__ rs = m_work(B, m);
    cplx* __restrict__ us = m_work(B, m) + uoff;
    cplx* scal = m_scal(B, m);
    if (threadIdx.x < 64) {
        const cplx rho = finish_in_wave(m_partial(B, m) + (int64_t)P_RHO * RED_BLOCKS, nb);
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
template <int NV>
__global__ __launch_bounds__(RED_THREADS) void k_bicg_rx(Members B, int64_t uoff, int nb, int cycle) {
    __shared__ cplx as; __shared__ int skip;
    const int m = B.m[blockIdx.y];
    const int64_t n = B.n, ld = B.n;
    cplx* __restrict__ rs = m_work(B, m);
    const cplx* __restrict__ us = m_work(B, m) + uoff;
    cplx* __restrict__ x = B.x + (int64_t)m * n;
    cplx* scal = m_scal(B, m);
    if (threadIdx.x < 64) {
        const cplx sg = finish_in_wave(m_partial(B, m) + (int64_t)P_SIGMA * RED_BLOCKS, nb);
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
__global__ __launch_bounds__(64) void k_mr_solve(Members B, int nb, int nv, int cycle) {
    __shared__ cplx G[NVMAX][NVMAX];
    const int m = B.m[blockIdx.y];
    const cplx* __restrict__ partial = m_partial(B, m);
    cplx* scal = m_scal(B, m);
    int e = 0;
    for (int a = 0; a < nv; ++a)
        for (int b = a; b < nv; ++b, ++e) {
            const cplx g = finish_in_wave(partial + (int64_t)(P_GRAM + e) * RED_BLOCKS, nb);
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
__global__ __launch_bounds__(64) void k_res_finish(Members B, int nb) {
    const int m = B.m[blockIdx.y];
    cplx* scal = m_scal(B, m);
    const cplx s = finish_in_wave(m_partial(B, m) + (int64_t)P_NORM * RED_BLOCKS, nb);
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

} // namespace

// nrhs solves in lock step.  x (in/out) and b: nrhs device vectors back to back; r_shadow (may be NULL): nrhs vectors of N
// complex on the device, or on the host (shadow_on_host); resnorm: nrhs rows of cap entries.  pc takes the active members
// of every round (Precond::apply).  code[2 j], code[2 j + 1]: LSFC_BICG_* of member j and its cycle (of the breakdown,
// else the last one).
static void bicgstabl_run(lsfc_plan* p, int nrhs, cplx* x, const cplx* b, const cplx* r_shadow, bool shadow_on_host, const Precond& pc,
                          const lsfc_bicgstabl_opts& o, int l, int64_t maxmv, double reltol, double abstol, double* resnorm, int64_t cap,
                          lsfc_gmres_result* res, int64_t* code) {
    const int64_t N = p->N;
    hipStream_t st = p->stream;
    const int nb = blas_red_blocks(N), nv = l + 1;
    const int64_t wstride = (int64_t)(2 * l + 3) * N, uoff = (int64_t)nv * N, toff = 2 * (int64_t)nv * N;
    DevBuf<cplx> work, scal, partial;
    DevBuf<double> tol2;
    work.alloc((size_t)nrhs * (size_t)wstride);
    scal.alloc((size_t)nrhs * S_COUNT);
    partial.alloc((size_t)nrhs * P_SLOTS * RED_BLOCKS);
    tol2.alloc((size_t)nrhs);
    auto R = [&](int m, int i) { return work.p + (size_t)m * (size_t)wstride + (size_t)i * N; };
    auto U = [&](int m, int i) { return R(m, nv + i); };
    Pinned hs, ht, vpin; hs.alloc((size_t)nrhs * S_COUNT); ht.alloc((size_t)(nrhs + 1) / 2);
    if (pc.fn && !pc.on_device) vpin.alloc((size_t)N);
    Event fetched; fetched.create();
    Members base{};
    base.work = work.p; base.x = x; base.scal = scal.p; base.partial = partial.p; base.tol2 = tol2.p; base.wstride = wstride; base.n = N;
    auto members = [&](const std::vector<int>& list) { Members B = base; for (size_t a = 0; a < list.size(); ++a) B.m[a] = list[a]; return B; };

    // the operator on vector `in(m)` of every member of the list, in groups that share one pass of the pipeline
    std::vector<const cplx*> av;
    std::vector<cplx*> pv;
    auto apply = [&](const std::vector<int>& list, auto&& in, auto&& out) {
        av.clear(); pv.clear();
        for (int m : list) { av.push_back(in(m)); pv.push_back(out(m)); }
        plan_apply_batch_dev(p, av.data(), pv.data(), list.size());
    };
    auto precondition = [&](const std::vector<int>& list, auto&& v) {
        pv.clear();
        for (int m : list) pv.push_back(v(m));
        pc.apply(pv.data(), pv.size(), vpin.p, st);
    };
    // all members' scalars in one copy
    auto fetch = [&]() {
        LSFC_HIP(hipMemcpyAsync(hs.p, scal.p, (size_t)nrhs * S_COUNT * sizeof(cplx), hipMemcpyDeviceToHost, st));
        LSFC_HIP(hipEventRecord(fetched.e, st));
        LSFC_HIP(hipEventSynchronize(fetched.e));
    };
    auto H = [&](int m) { return hs.p + (size_t)m * S_COUNT; };
    // scal[S_RES] = ||rs[0]|| of the members of the list
    auto norm0 = [&](const std::vector<int>& list) {
        const Members B = members(list);
        hipLaunchKernelGGL(k_dot, dim3(nb, (unsigned)list.size()), dim3(RED_THREADS), 0, st, B, (int64_t)0, (int64_t)0, (int)P_NORM);
        hipLaunchKernelGGL(k_norm_finish, dim3(1, (unsigned)list.size()), dim3(64), 0, st, B, nb);
    };

    // init: rs[0] = Pl \ (b - A x), us = 0, shadow residual, sigma = -1 (sigma = 1, negated by the first cycle)
    std::vector<Solve> S((size_t)nrhs);
    std::vector<int> act((size_t)nrhs);
    for (int m = 0; m < nrhs; ++m) act[(size_t)m] = m;
    if (o.initially_zero) {
        for (int m = 0; m < nrhs; ++m) LSFC_HIP(hipMemcpyAsync(R(m, 0), b + (size_t)m * N, (size_t)N * sizeof(cplx), hipMemcpyDeviceToDevice, st));
    } else {
        apply(act, [&](int m) { return (const cplx*)(x + (size_t)m * N); }, [&](int m) { return R(m, 0); });
        hipLaunchKernelGGL(k_residual, dim3(grid_for(N), (unsigned)nrhs), dim3(256), 0, st, members(act), b);
        for (auto& s : S) s.mvps = 1;
    }
    precondition(act, [&](int m) { return R(m, 0); });
    for (int m = 0; m < nrhs; ++m) {
        LSFC_HIP(hipMemsetAsync(U(m, 0), 0, (size_t)nv * (size_t)N * sizeof(cplx), st));
        const cplx* sh = r_shadow ? r_shadow + (size_t)m * N : R(m, 0);
        LSFC_HIP(hipMemcpyAsync(R(m, 2 * nv), sh, (size_t)N * sizeof(cplx), r_shadow && shadow_on_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
    }
    for (size_t i = 0; i < (size_t)nrhs * S_COUNT; ++i) hs.p[i] = make_double2(0.0, 0.0);
    for (int m = 0; m < nrhs; ++m) H(m)[S_SIGMA] = make_double2(-1.0, 0.0);
    LSFC_HIP(hipMemcpyAsync(scal.p, hs.p, (size_t)nrhs * S_COUNT * sizeof(cplx), hipMemcpyHostToDevice, st));
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
    LSFC_HIP(hipMemcpyAsync(tol2.p, t2, (size_t)nrhs * sizeof(double), hipMemcpyHostToDevice, st));
    auto running = [&](const Solve& s) { return !s.converged && s.bad == ST_OK && s.mvps < maxmv; };
    auto still_active = [&]() { std::vector<int> a; for (int m = 0; m < nrhs; ++m) if (running(S[(size_t)m])) a.push_back(m); return a; };
    act = still_active();
    std::vector<int> broke;

    // every member of the list is in the same cycle: all start at 0 and a member never rejoins
    for (int64_t cycles = 0; !act.empty(); ++cycles) {
        const int cyc = (int)std::min<int64_t>(cycles + 1, 1 << 30);
        const Members B = members(act);
        const dim3 grid((unsigned)nb, (unsigned)act.size()), one(1, (unsigned)act.size());
        for (int j = 0; j < l; ++j) {                       // BiCG part
            hipLaunchKernelGGL(k_dot, grid, dim3(RED_THREADS), 0, st, B, toff, (int64_t)j * N, (int)P_RHO);
            dispatch<1, LMAX>(j + 1, "bicgstabl", [&](auto nvj) {
                hipLaunchKernelGGL((k_bicg_u<decltype(nvj)::value>), grid, dim3(RED_THREADS), 0, st, B, uoff, nb, cyc);
            });
            apply(act, [&](int m) { return (const cplx*)U(m, j); }, [&](int m) { return U(m, j + 1); });
            precondition(act, [&](int m) { return U(m, j + 1); });
            hipLaunchKernelGGL(k_dot, grid, dim3(RED_THREADS), 0, st, B, toff, uoff + (int64_t)(j + 1) * N, (int)P_SIGMA);
            dispatch<1, LMAX>(j + 1, "bicgstabl", [&](auto nvj) {
                hipLaunchKernelGGL((k_bicg_rx<decltype(nvj)::value>), grid, dim3(RED_THREADS), 0, st, B, uoff, nb, cyc);
            });
            apply(act, [&](int m) { return (const cplx*)R(m, j); }, [&](int m) { return R(m, j + 1); });
            precondition(act, [&](int m) { return R(m, j + 1); });
        }
        dispatch<2, NVMAX>(nv, "bicgstabl", [&](auto nvc) {              // MR part
            hipLaunchKernelGGL((k_gram<decltype(nvc)::value>), grid, dim3(RED_THREADS), 0, st, B);
        });
        hipLaunchKernelGGL(k_mr_solve, one, dim3(64), 0, st, B, nb, nv, cyc);
        dispatch<1, LMAX>(l, "bicgstabl", [&](auto lc) {
            hipLaunchKernelGGL((k_mr_update<decltype(lc)::value>), grid, dim3(RED_THREADS), 0, st, B, uoff);
        });
        hipLaunchKernelGGL(k_res_finish, one, dim3(64), 0, st, B, nb);
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
    LSFC_HIP(hipStreamSynchronize(st));
    for (int m = 0; m < nrhs; ++m) {
        const Solve& s = S[(size_t)m];
        res[m].iters = s.cycles; res[m].mvps = s.mvps; res[m].converged = s.converged ? 1 : 0; res[m].final_resnorm = s.current;
        code[2 * m] = s.converged ? LSFC_BICG_CONVERGED : (s.bad != ST_OK ? s.bad : LSFC_BICG_MAX_MV);
        code[2 * m + 1] = (!s.converged && s.bad != ST_OK) ? s.bad_cycle : s.cycles;
    }
}

// the argument checks of both entry points, before any device call
static void check_args(const char* fn, lsfc_plan* plan, const double* x, const double* b, const lsfc_bicgstabl_opts* opts, const double* resnorm,
                       int64_t resnorm_cap, const lsfc_gmres_result* result, int memspace) {
    LSFC_REQUIRE(opts, "%s: NULL opts", fn);
    LSFC_REQUIRE(opts->l >= 1 && opts->l <= LMAX, "%s: l = %d is outside 1..%d", fn, opts->l, LMAX);
    for (int i = 0; i < 4; ++i) LSFC_REQUIRE(opts->reserved[i] == 0, "%s: reserved[%d] is not zero", fn, i);
    LSFC_REQUIRE(memspace == LSFC_MEM_HOST || memspace == LSFC_MEM_DEVICE, "%s: unknown memspace %d", fn, memspace);
    LSFC_REQUIRE(plan && x && b && result, "%s: NULL argument", fn);
    LSFC_REQUIRE(resnorm || resnorm_cap <= 0, "%s: NULL resnorm with a capacity of %lld", fn, (long long)resnorm_cap);
    LSFC_REQUIRE(!plan->multi && !plan->dist, "%s runs on a single-device plan (not a distributed or multi-device one)", fn);
}

} // namespace lsfc

using namespace lsfc;

// Both entry points (defined below them): the argument checks, the option defaults, the memory rule (nrhs (2 l + 3) work vectors; host vectors:
// the staged x and b, 2 nrhs vectors, on top -- r_shadow is uploaded into its work vector), host staging through
// plan->xs / plan->ys, and the solve.  batch: the texts of lsfc_bicgstabl_batch, and its members meet at the library's
// own preconditioner; the single call has nobody to meet there and calls the callback as given.
static void bicgstabl_entry(const char* fn, bool batch, lsfc_plan* plan, double* x, const double* b, int64_t nrhs, const lsfc_bicgstabl_opts* opts,
                            double* resnorm, int64_t resnorm_cap, lsfc_gmres_result* results, int64_t* code, int memspace);

extern "C" int lsfc_bicgstabl(lsfc_plan* plan, double* x, const double* b, const lsfc_bicgstabl_opts* opts, double* resnorm,
                              int64_t resnorm_cap, lsfc_gmres_result* result, int memspace) {
    int64_t code[2] = { 0, 0 };
    const int rc = guarded([&] { bicgstabl_entry("lsfc_bicgstabl", false, plan, x, b, 1, opts, resnorm, resnorm_cap, result, code, memspace); });
    if (rc != LSFC_OK || result->converged) return rc;
    if (code[0] != LSFC_BICG_MAX_MV) set_last_error("bicgstabl: breakdown in cycle %d: %s; x is the last finite iterate", (int)code[1], ST_NAME[code[0]]);
    else set_last_error("bicgstabl: max_mv_products reached without convergence");
    return LSFC_ENOTCONV;
}

extern "C" int lsfc_bicgstabl_batch(lsfc_plan* plan, double* x, const double* b, int64_t nrhs, const lsfc_bicgstabl_opts* opts, double* resnorm,
                                    int64_t resnorm_cap, lsfc_gmres_result* results, int64_t* status, int memspace) {
    int64_t code[2 * KRYLOV_NRHS_MAX] = { 0 };
    const int rc = guarded([&] {
        bicgstabl_entry("lsfc_bicgstabl_batch", true, plan, x, b, nrhs, opts, resnorm, resnorm_cap, results, code, memspace);
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

static void bicgstabl_entry(const char* fn, bool batch, lsfc_plan* plan, double* x, const double* b, int64_t nrhs, const lsfc_bicgstabl_opts* opts,
                            double* resnorm, int64_t resnorm_cap, lsfc_gmres_result* results, int64_t* code, int memspace) {
    if (batch) LSFC_REQUIRE(nrhs >= 1 && nrhs <= KRYLOV_NRHS_MAX, "%s: nrhs = %lld is outside 1..%d", fn, (long long)nrhs, KRYLOV_NRHS_MAX);
    check_args(fn, plan, x, b, opts, resnorm, resnorm_cap, results, memspace);
    const int l = opts->l, n = (int)nrhs;
    const int64_t N = plan->N;
    const int64_t maxmv = opts->max_mv_products > 0 ? opts->max_mv_products : N;
    const double reltol = opts->reltol >= 0 ? opts->reltol : DEFAULT_RELTOL;
    const double abstol = opts->abstol > 0 ? opts->abstol : 0.0;
    plan_check_precond_op(plan, opts->precond, opts->precond_user, fn);
    const Precond pc(opts->precond, opts->precond_user, opts->precond_on_device != 0, batch, N, fn);
    LSFC_HIP(hipSetDevice(plan->device));
    const bool host = memspace == LSFC_MEM_HOST;
    const bool stage = host && plan->xs.n < (size_t)n * (size_t)N;
    {
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
    }
    const cplx* xd = (const cplx*)x; const cplx* bd = (const cplx*)b;
    const size_t bytes = (size_t)n * (size_t)N * sizeof(cplx);
    if (host) {
        if (stage) { plan->xs.alloc((size_t)n * (size_t)N); plan->ys.alloc((size_t)n * (size_t)N); }     // (plan_ensure_staging, with the `stage` the memory rule counted)
        LSFC_HIP(hipMemcpy(plan->xs.p, x, bytes, hipMemcpyHostToDevice));
        LSFC_HIP(hipMemcpy(plan->ys.p, b, bytes, hipMemcpyHostToDevice));
        xd = plan->xs.p; bd = plan->ys.p;
    }
    bicgstabl_run(plan, n, (cplx*)xd, bd, (const cplx*)opts->r_shadow, host, pc, *opts, l, maxmv, reltol, abstol, resnorm,
                  resnorm_cap > 0 ? resnorm_cap : 0, results, code);
    if (host) LSFC_HIP(hipMemcpy(x, plan->xs.p, bytes, hipMemcpyDeviceToHost));
}
