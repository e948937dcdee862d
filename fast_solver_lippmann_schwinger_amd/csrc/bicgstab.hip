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
#include "plan.hpp"
#include "pointwise.hpp"
#include "reduce.hpp"
#include <cmath>
#include <type_traits>

namespace lsfc {
namespace {

constexpr int LMAX = 8, NVMAX = LMAX + 1;
// device scalars (cplx each)
enum { S_RHO = 0, S_SIGMA = 1, S_BETA = 2, S_ALPHA = 3, S_STATUS = 4 /* (code, cycle) */, S_RES = 5, S_GAMMA = 6 /* LMAX */,
       S_G = 16 /* NVMAX * NVMAX, row-major */, S_COUNT = 16 + NVMAX * NVMAX };
enum { ST_OK = 0, ST_EXHAUSTED = 1, ST_RHO = 2, ST_SIGMA = 3, ST_BETA = 4, ST_ALPHA = 5, ST_GAMMA = 6, ST_RESIDUAL = 7 };
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
// a - c * b
__device__ __forceinline__ cplx csubmul(cplx a, cplx c, cplx b) {
    return make_double2(a.x - fma(c.x, b.x, -c.y * b.y), a.y - fma(c.x, b.y, c.y * b.x));
}
__device__ __forceinline__ cplx caddmul(cplx a, cplx c, cplx b) {
    return make_double2(a.x + fma(c.x, b.x, -c.y * b.y), a.y + fma(c.x, b.y, c.y * b.x));
}

// y = b - y  (initial residual from y = A x)
__global__ void k_residual(cplx* __restrict__ y, const cplx* __restrict__ b, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const cplx u = b[i], v = y[i]; y[i] = make_double2(u.x - v.x, u.y - v.y);
    }
}

// rho = sum(rpartial[0..nb)), beta = rho / sigma; us[i] = rs[i] - beta us[i] for i < NV (= j + 1); block 0 publishes rho, beta
template <int NV>
__global__ __launch_bounds__(RED_THREADS) void k_bicg_u(cplx* __restrict__ us, const cplx* __restrict__ rs, int64_t ld, const cplx* __restrict__ rpartial,
                                                         int nb, cplx* scal, int cycle, int64_t n) {
    __shared__ cplx bs; __shared__ int skip;
    if (threadIdx.x < 64) {
        const cplx rho = finish_in_wave(rpartial, nb);
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

// sigma = sum(spartial[0..nb)), alpha = rho / sigma; rs[i] -= alpha us[i+1] for i < NV (= j + 1), x += alpha us[0];
// block 0 publishes sigma, alpha
template <int NV>
__global__ __launch_bounds__(RED_THREADS) void k_bicg_rx(cplx* __restrict__ rs, const cplx* __restrict__ us, cplx* __restrict__ x, int64_t ld,
                                                          const cplx* __restrict__ spartial, int nb, cplx* scal, int cycle, int64_t n) {
    __shared__ cplx as; __shared__ int skip;
    if (threadIdx.x < 64) {
        const cplx sg = finish_in_wave(spartial, nb);
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
__global__ __launch_bounds__(RED_THREADS) void k_gram(const cplx* __restrict__ rs, int64_t ld, cplx* __restrict__ partial, int64_t n) {
    __shared__ cplx sh[RED_THREADS / 64];
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
            acc[e].x = fma(v[a].x, v[a].x, fma(v[a].y, v[a].y, acc[e].x));      // the diagonal is real
            ++e;
#pragma unroll
            for (int b = a + 1; b < NV; ++b, ++e) {
                acc[e].x = fma(v[a].x, v[b].x, fma(v[a].y, v[b].y, acc[e].x));
                acc[e].y = fma(v[a].x, v[b].y, fma(-v[a].y, v[b].x, acc[e].y));
            }
        }
    }
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const cplx r = block_sum(acc[e], sh);
        if (threadIdx.x == 0) partial[(int64_t)(P_GRAM + e) * RED_BLOCKS + blockIdx.x] = r;
        __syncthreads();
    }
}

// One wave.  G from the partials (published in scal[S_G..], row-major NVMAX x NVMAX); G[0,0] <= tol^2: the Krylov space is
// exhausted, status ST_EXHAUSTED and no solve of a singular G.  Otherwise gamma = G[1:,1:] \ G[1:,0] by LU with partial
// pivoting (largest |.|^2 of the column, the lowest row on a tie) and sigma = -(sigma gamma_{l-1}): the factor of the MR
// part and the sign flip that opens the next cycle.
__global__ __launch_bounds__(64) void k_mr_solve(const cplx* __restrict__ partial, int nb, int nv, cplx* scal, double tol2, int cycle) {
    __shared__ cplx G[NVMAX][NVMAX];
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
    if (G[0][0].x <= tol2) { scal[S_STATUS] = make_double2((double)ST_EXHAUSTED, (double)cycle); return; }
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
__global__ __launch_bounds__(RED_THREADS) void k_mr_update(cplx* __restrict__ us, cplx* __restrict__ rs, cplx* __restrict__ x, int64_t ld,
                                                            const cplx* __restrict__ scal, cplx* __restrict__ partial, int64_t n) {
    __shared__ cplx sh[RED_THREADS / 64];
    __shared__ cplx gs[L];
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
        nrm.x = fma(r0.x, r0.x, fma(r0.y, r0.y, nrm.x));
    }
    const cplx s = block_sum(nrm, sh);
    if (threadIdx.x == 0) partial[(int64_t)P_NORM * RED_BLOCKS + blockIdx.x] = s;
}

// scal[S_RES] = sqrt(sum of the P_NORM partials), unless the cycle ended without an MR update
__global__ __launch_bounds__(64) void k_res_finish(const cplx* __restrict__ partial, int nb, cplx* scal) {
    const cplx s = finish_in_wave(partial + (int64_t)P_NORM * RED_BLOCKS, nb);
    if (threadIdx.x == 0 && scal[S_STATUS].x == 0.0) scal[S_RES] = make_double2(sqrt(s.x), 0.0);
}

template <int LO, int HI, class F> void dispatch(int v, F&& f) {
    if constexpr (LO > HI) fail(LSFC_EINVAL, "bicgstabl: no kernel for %d vectors", v);
    else if (v == LO) f(std::integral_constant<int, LO>{});
    else dispatch<LO + 1, HI>(v, f);
}

inline unsigned ew_grid(int64_t n) {
    const int64_t g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
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

} // namespace

// x (in/out) and b: device vectors; r_shadow (may be NULL): N complex on the device, or on the host (shadow_on_host).  Returns the breakdown code (ST_OK: none) and its cycle.
static int bicgstabl_run(lsfc_plan* p, cplx* x, const cplx* b, const cplx* r_shadow, bool shadow_on_host, const lsfc_bicgstabl_opts& o, int l, int64_t maxmv,
                         double reltol, double abstol, double* resnorm, int64_t cap, lsfc_gmres_result* res, int* bad_cycle) {
    const int64_t N = p->N;
    hipStream_t st = p->stream;
    const int nb = blas_red_blocks(N), nv = l + 1;
    DevBuf<cplx> work, scal, partial;
    work.alloc((size_t)(2 * l + 3) * (size_t)N);
    scal.alloc(S_COUNT);
    partial.alloc((size_t)P_SLOTS * RED_BLOCKS);
    cplx* rs = work.p; cplx* us = rs + (size_t)nv * N; cplx* rt = us + (size_t)nv * N;
    auto R = [&](int i) { return rs + (size_t)i * N; };
    auto U = [&](int i) { return us + (size_t)i * N; };
    auto slot = [&](int s) { return partial.p + (size_t)s * RED_BLOCKS; };
    Pinned hs, vpin; hs.alloc(S_COUNT);
    const bool host_cb = o.precond && !o.precond_on_device;
    if (host_cb) vpin.alloc((size_t)N);
    Event fetched; fetched.create();

    auto precondition = [&](cplx* v) {
        if (!o.precond) return;
        if (o.precond_on_device) {
            const int rc = o.precond(o.precond_user, (double*)v, N);
            if (rc != 0) fail(LSFC_EINVAL, "preconditioner callback returned %d", rc);
            return;
        }
        LSFC_HIP(hipMemcpyAsync(vpin.p, v, (size_t)N * sizeof(cplx), hipMemcpyDeviceToHost, st));
        LSFC_HIP(hipStreamSynchronize(st));
        const int rc = o.precond(o.precond_user, (double*)vpin.p, N);
        if (rc != 0) fail(LSFC_EINVAL, "preconditioner callback returned %d", rc);
        LSFC_HIP(hipMemcpyAsync(v, vpin.p, (size_t)N * sizeof(cplx), hipMemcpyHostToDevice, st));
    };
    auto fetch = [&]() {
        LSFC_HIP(hipMemcpyAsync(hs.p, scal.p, (size_t)S_COUNT * sizeof(cplx), hipMemcpyDeviceToHost, st));
        LSFC_HIP(hipEventRecord(fetched.e, st));
        LSFC_HIP(hipEventSynchronize(fetched.e));
    };

    // init: rs[0] = Pl \ (b - A x), us = 0, shadow residual, sigma = -1 (sigma = 1, negated by the first cycle)
    int64_t mvps = 0;
    if (o.initially_zero) LSFC_HIP(hipMemcpyAsync(R(0), b, (size_t)N * sizeof(cplx), hipMemcpyDeviceToDevice, st));
    else {
        plan_apply_dev(p, x, R(0));
        hipLaunchKernelGGL(k_residual, dim3(ew_grid(N)), dim3(256), 0, st, R(0), b, N);
        mvps = 1;
    }
    precondition(R(0));
    LSFC_HIP(hipMemsetAsync(us, 0, (size_t)nv * (size_t)N * sizeof(cplx), st));
    if (r_shadow && shadow_on_host) LSFC_HIP(hipMemcpyAsync(rt, r_shadow, (size_t)N * sizeof(cplx), hipMemcpyHostToDevice, st));
    else LSFC_HIP(hipMemcpyAsync(rt, r_shadow ? r_shadow : R(0), (size_t)N * sizeof(cplx), hipMemcpyDeviceToDevice, st));
    LSFC_HIP(hipMemsetAsync(scal.p, 0, (size_t)S_COUNT * sizeof(cplx), st));
    static const cplx minus_one = { -1.0, 0.0 };
    LSFC_HIP(hipMemcpyAsync(scal.p + S_SIGMA, &minus_one, sizeof(cplx), hipMemcpyHostToDevice, st));
    blas_nrm2(R(0), slot(P_NORM), scal.p + S_RES, N, st);
    fetch();
    const double beta0 = hs.p[S_RES].x;
    const double tol = std::max(reltol * beta0, abstol);
    double current = beta0;
    bool converged = beta0 <= tol;
    int bad = std::isfinite(beta0) ? ST_OK : ST_RESIDUAL;
    *bad_cycle = 0;
    int64_t cycles = 0;

    while (!converged && bad == ST_OK && mvps < maxmv) {
        const int cyc = (int)std::min<int64_t>(cycles + 1, 1 << 30);
        for (int j = 0; j < l; ++j) {                       // BiCG part
            blas_dot_partial(rt, R(j), slot(P_RHO), N, st);
            dispatch<1, LMAX>(j + 1, [&](auto nvj) {
                hipLaunchKernelGGL((k_bicg_u<decltype(nvj)::value>), dim3(nb), dim3(RED_THREADS), 0, st, us, (const cplx*)rs, N, (const cplx*)slot(P_RHO), nb, scal.p, cyc, N);
            });
            plan_apply_dev(p, U(j), U(j + 1));
            precondition(U(j + 1));
            blas_dot_partial(rt, U(j + 1), slot(P_SIGMA), N, st);
            dispatch<1, LMAX>(j + 1, [&](auto nvj) {
                hipLaunchKernelGGL((k_bicg_rx<decltype(nvj)::value>), dim3(nb), dim3(RED_THREADS), 0, st, rs, (const cplx*)us, x, N, (const cplx*)slot(P_SIGMA), nb, scal.p, cyc, N);
            });
            plan_apply_dev(p, R(j), R(j + 1));
            precondition(R(j + 1));
            mvps += 2;
        }
        dispatch<2, NVMAX>(nv, [&](auto nvc) {              // MR part
            hipLaunchKernelGGL((k_gram<decltype(nvc)::value>), dim3(nb), dim3(RED_THREADS), 0, st, (const cplx*)rs, N, partial.p, N);
        });
        hipLaunchKernelGGL(k_mr_solve, dim3(1), dim3(64), 0, st, (const cplx*)partial.p, nb, nv, scal.p, tol * tol, cyc);
        dispatch<1, LMAX>(l, [&](auto lc) {
            hipLaunchKernelGGL((k_mr_update<decltype(lc)::value>), dim3(nb), dim3(RED_THREADS), 0, st, us, rs, x, N, (const cplx*)scal.p, partial.p, N);
        });
        hipLaunchKernelGGL(k_res_finish, dim3(1), dim3(64), 0, st, (const cplx*)partial.p, nb, scal.p);
        LSFC_HIP(hipGetLastError());
        fetch();
        const int status = (int)hs.p[S_STATUS].x;
        if (status == ST_OK) {
            current = hs.p[S_RES].x;
            if (!std::isfinite(current)) { bad = ST_RESIDUAL; *bad_cycle = cyc; }
        } else if (status == ST_EXHAUSTED) {
            current = std::sqrt(hs.p[S_G].x);
            converged = true;
        } else {
            // breakdown: x and rs[0] are the last finite pair -- the residual of that iterate decides (a breakdown with
            // the residual already below the tolerance is the exhausted Krylov space met one step early)
            bad = status; *bad_cycle = (int)hs.p[S_STATUS].y;
            blas_nrm2(R(0), slot(P_NORM), scal.p + S_RES, N, st);
            fetch();
            current = hs.p[S_RES].x;
        }
        if (resnorm && cycles < cap) resnorm[cycles] = current;
        ++cycles;
        converged = converged || current <= tol;
    }
    LSFC_HIP(hipStreamSynchronize(st));
    res->iters = cycles; res->mvps = mvps; res->converged = converged ? 1 : 0; res->final_resnorm = current;
    return converged ? ST_OK : bad;
}

} // namespace lsfc

using namespace lsfc;

extern "C" int lsfc_bicgstabl(lsfc_plan* plan, double* x, const double* b, const lsfc_bicgstabl_opts* opts, double* resnorm,
                              int64_t resnorm_cap, lsfc_gmres_result* result, int memspace) {
    int bad = ST_OK, bad_cycle = 0; bool notconv = false;
    const int rc = guarded([&] {
        // argument checks, before any device call
        LSFC_REQUIRE(opts, "lsfc_bicgstabl: NULL opts");
        LSFC_REQUIRE(opts->l >= 1 && opts->l <= LMAX, "lsfc_bicgstabl: l = %d is outside 1..%d", opts->l, LMAX);
        for (int i = 0; i < 4; ++i) LSFC_REQUIRE(opts->reserved[i] == 0, "lsfc_bicgstabl: reserved[%d] is not zero", i);
        LSFC_REQUIRE(memspace == LSFC_MEM_HOST || memspace == LSFC_MEM_DEVICE, "lsfc_bicgstabl: unknown memspace %d", memspace);
        LSFC_REQUIRE(plan && x && b && result, "lsfc_bicgstabl: NULL argument");
        LSFC_REQUIRE(resnorm || resnorm_cap <= 0, "lsfc_bicgstabl: NULL resnorm with a capacity of %lld", (long long)resnorm_cap);
        LSFC_REQUIRE(!plan->multi && !plan->dist, "lsfc_bicgstabl runs on a single-device plan (not a distributed or multi-device one)");
        const int l = opts->l;
        const int64_t N = plan->N;
        const int64_t maxmv = opts->max_mv_products > 0 ? opts->max_mv_products : N;
        const double reltol = opts->reltol >= 0 ? opts->reltol : std::sqrt(2.220446049250313e-16);
        const double abstol = opts->abstol > 0 ? opts->abstol : 0.0;
        LSFC_HIP(hipSetDevice(plan->device));
        // memory rule: 2 l + 3 work vectors; host vectors: the staged x and b on top (r_shadow is uploaded into its work vector)
        const bool host = memspace == LSFC_MEM_HOST;
        const bool stage = host && plan->xs.n < (size_t)N;
        {
            size_t free_b = 0, total_b = 0;
            LSFC_HIP(hipMemGetInfo(&free_b, &total_b));
            const double need = ((double)(2 * l + 3) + (stage ? 2.0 : 0.0)) * (double)N * sizeof(cplx);
            if (need > (double)free_b)
                fail(LSFC_ENOMEM, "lsfc_bicgstabl: (2 l + 3 = %d work vectors%s) of %lld complex need %.1f GB of device memory, %.1f GB are free "
                     "-- lower l", 2 * l + 3, stage ? " + staged x and b" : "", (long long)N, need / 1e9, (double)free_b / 1e9);
        }
        const cplx* xd = (const cplx*)x; const cplx* bd = (const cplx*)b; const cplx* sd = (const cplx*)opts->r_shadow;
        if (host) {
            if (stage) { plan->xs.alloc((size_t)N); plan->ys.alloc((size_t)N); }
            LSFC_HIP(hipMemcpy(plan->xs.p, x, (size_t)N * sizeof(cplx), hipMemcpyHostToDevice));
            LSFC_HIP(hipMemcpy(plan->ys.p, b, (size_t)N * sizeof(cplx), hipMemcpyHostToDevice));
            xd = plan->xs.p; bd = plan->ys.p;
        }
        bad = bicgstabl_run(plan, (cplx*)xd, bd, sd, host, *opts, l, maxmv, reltol, abstol, resnorm, resnorm_cap > 0 ? resnorm_cap : 0, result, &bad_cycle);
        if (host) LSFC_HIP(hipMemcpy(x, plan->xs.p, (size_t)N * sizeof(cplx), hipMemcpyDeviceToHost));
        notconv = !result->converged;
    });
    if (rc != LSFC_OK || !notconv) return rc;
    if (bad != ST_OK) set_last_error("bicgstabl: breakdown in cycle %d: %s; x is the last finite iterate", bad_cycle, ST_NAME[bad]);
    else set_last_error("bicgstabl: max_mv_products reached without convergence");
    return LSFC_ENOTCONV;
}
