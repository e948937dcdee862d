// Off-grid sources and receivers: the sampling operator R (nrecv x N, dense, never stored) between grid vectors and point
// receivers or far-field directions, its transpose and its adjoint (lsfc_receivers_*; DESIGN.md section 3, "Off-grid sources and
// receivers").  Row r of R is the free-space Green's function of the reference, weighted by h^d (src/FastConvolution3D.jl:188,
// src/FastConvolution.jl:268), between receiver r and every grid point, or its far-field limit in direction r.
//
//   forward (N)   every thread keeps RECV_RT receivers x NB members of sums in registers and walks a grid-stride slice of the points;
//                 the Green's function is evaluated once per (point, receiver) for all members.  Block partials, then one wave per
//                 (member, receiver) adds them in index order: the two-stage reduction of reduce.hpp.
//   far field     e^{-ik theta.x_i} = Ex[ix] Ey[iy] Ez[iz] from three tables per direction built at create time; the loop over a
//                 line of x has no transcendental.
//   T / H         one thread per grid point; receivers are staged through LDS RECV_CHUNK at a time and added in receiver order.
// No atomics, no host work inside an apply; every sum has one fixed order, so the bits of one receiver's (one point's) and one
// member's result depend on nothing but its own inputs.
#include "plan.hpp"
#include "receivers.hpp"
#include "reduce.hpp"
#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

struct lsfc_receivers {
    int device = 0;
    hipStream_t stream = nullptr;
    int ndim = 3, kind = LSFC_RECV_POINTS;
    int dims[3] = {1, 1, 1};
    double origin[3] = {0.0, 0.0, 0.0}, h = 0.0, k = 0.0;
    int64_t N = 0, nrecv = 0;
    lsfc::DevBuf<double> coords;          // points: nrecv x 3 (z = 0 in 2D)
    lsfc::DevBuf<lsfc::cplx> tab;         // far field: nrecv x (n + m + l), e^{-ik theta_a (o_a + h i)} of axis a = x, y, z back to back
    lsfc::DevBuf<lsfc::cplx> partial;     // block partials of the forward kernels, grown on first use
    lsfc::DevBuf<lsfc::cplx> hin, hout;   // staging of host vectors, grown on first use
};

namespace lsfc {
namespace {

struct Geo { int n, m, l; double ox, oy, oz, h, k, amp; };   // amp: h^3 / (4 pi) in 3D, h^2 / 4 in 2D (points)
struct Stride { int sx, sy, sz; };                          // the grid stride of the forward kernel as (x, y, z) steps
// the fused medium: nu == nullptr without a plan; else the vector is multiplied by scale * nu (scale = -omega^2)
struct Medium { const double* nu; const double* nu_im; double scale; };

__device__ __forceinline__ cplx cmul(cplx a, cplx b) { return make_double2(fma(a.x, b.x, -(a.y * b.y)), fma(a.x, b.y, a.y * b.x)); }
// acc += g * q
__device__ __forceinline__ void cfma(cplx& acc, cplx g, cplx q) {
    acc.x = fma(g.x, q.x, fma(-g.y, q.y, acc.x));
    acc.y = fma(g.x, q.y, fma(g.y, q.x, acc.y));
}
// the factor scale * nu_i (or its conjugate) of grid point i, and its product with v; a real nu keeps to real multiplies
__device__ __forceinline__ cplx medium_factor(const Medium& md, int64_t i, bool conj) {
    const double a = md.scale * md.nu[i];
    if (!md.nu_im) return make_double2(a, 0.0);
    const double b = md.scale * md.nu_im[i];
    return make_double2(a, conj ? -b : b);
}
__device__ __forceinline__ cplx medium_mul(const Medium& md, cplx f, cplx v) {
    return md.nu_im ? cmul(f, v) : make_double2(f.x * v.x, f.x * v.y);
}

// h^d G(d) for the offset d between a receiver and a grid point
template <int DIM> __device__ __forceinline__ cplx green(const Geo& g, double dx, double dy, double dz) {
    if constexpr (DIM == 3) {
        const double r2 = fma(dx, dx, fma(dy, dy, dz * dz));
        const double rinv = rsqrt(r2), r = r2 * rinv;
        double sn, cs; sincos(g.k * r, &sn, &cs);
        const double a = g.amp * rinv;
        return make_double2(a * cs, a * sn);
    } else {
        const double kr = g.k * sqrt(fma(dx, dx, dy * dy));
        return make_double2(-g.amp * y0(kr), g.amp * j0(kr));      // (i/4) (J0 + i Y0)
    }
}

// the block's sums of RT x NB accumulators -> partial[(member * rpass + receiver) * blocks + block]
template <int NB> __device__ __forceinline__ void store_partials(cplx (&acc)[RECV_RT][NB], int r0, int nrecv, int rpass, cplx* __restrict__ partial) {
    __shared__ cplx sh[RECV_RT * NB][RED_THREADS / 64];
#pragma unroll
    for (int t = 0; t < RECV_RT; ++t)
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const cplx s = block_sum(acc[t][j], sh[t * NB + j]);
            if (threadIdx.x == 0 && r0 + t < nrecv) partial[((size_t)j * rpass + (r0 + t)) * gridDim.x + blockIdx.x] = s;
        }
}

// forward, point receivers: this block's slice of sum_i g(p_r, x_i) q_j[i] for RECV_RT receivers and NB members
template <int DIM, int NB> __global__ __launch_bounds__(RED_THREADS)
void k_recv_fwd_points(Geo g, Stride st, Medium md, const double* __restrict__ coords, int nrecv, int rpass,
                       const cplx* __restrict__ q, int64_t N, cplx* __restrict__ partial) {
    const int r0 = blockIdx.y * RECV_RT;
    // wave-uniform: the same receivers for every lane (a tail chunk repeats the last receiver and stores nothing for the repeats)
    double px[RECV_RT], py[RECV_RT], pz[RECV_RT];
#pragma unroll
    for (int t = 0; t < RECV_RT; ++t) {
        const int r = min(r0 + t, nrecv - 1);
        px[t] = coords[3 * r]; py[t] = coords[3 * r + 1]; pz[t] = coords[3 * r + 2];
    }
    cplx acc[RECV_RT][NB];
#pragma unroll
    for (int t = 0; t < RECV_RT; ++t)
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[t][j] = make_double2(0.0, 0.0);
    int64_t i = (int64_t)blockIdx.x * RED_THREADS + threadIdx.x;
    const int64_t step = (int64_t)gridDim.x * RED_THREADS;
    int ix = (int)(i % g.n), iy = (int)((i / g.n) % g.m), iz = (int)(i / ((int64_t)g.n * g.m));
    if constexpr (DIM == 2) { iy = (int)(i / g.n); iz = 0; }
    for (; i < N; i += step) {
        const double x = fma(g.h, (double)ix, g.ox), y = fma(g.h, (double)iy, g.oy), z = DIM == 3 ? fma(g.h, (double)iz, g.oz) : 0.0;
        cplx qv[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) qv[j] = q[(size_t)j * N + i];
        if (md.nu) {
            const cplx f = medium_factor(md, i, false);
#pragma unroll
            for (int j = 0; j < NB; ++j) qv[j] = medium_mul(md, f, qv[j]);
        }
#pragma unroll
        for (int t = 0; t < RECV_RT; ++t) {
            const cplx gv = green<DIM>(g, px[t] - x, py[t] - y, pz[t] - z);
#pragma unroll
            for (int j = 0; j < NB; ++j) cfma(acc[t][j], gv, qv[j]);
        }
        // the next point of the slice, without a division
        ix += st.sx; if (ix >= g.n) { ix -= g.n; ++iy; }
        iy += st.sy;
        if constexpr (DIM == 3) { if (iy >= g.m) { iy -= g.m; ++iz; } iz += st.sz; }
    }
    store_partials<NB>(acc, r0, nrecv, rpass, partial);
}

// forward, far field: tab + r * (n + m + l) holds Ex, Ey, Ez of direction r.  1 << xshift lanes share a line of x; the block takes
// RED_THREADS >> xshift lines at a time
template <int DIM, int NB> __global__ __launch_bounds__(RED_THREADS)
void k_recv_fwd_far(Geo g, int xshift, Medium md, const cplx* __restrict__ tab, int nrecv, int rpass,
                    const cplx* __restrict__ q, int64_t N, cplx* __restrict__ partial) {
    const int r0 = blockIdx.y * RECV_RT;
    const int xt = threadIdx.x & ((1 << xshift) - 1), lt = threadIdx.x >> xshift, xstep = 1 << xshift, lp = RED_THREADS >> xshift;
    const int tl = g.n + g.m + g.l;
    const cplx* T[RECV_RT];
#pragma unroll
    for (int t = 0; t < RECV_RT; ++t) T[t] = tab + (size_t)min(r0 + t, nrecv - 1) * tl;
    cplx acc[RECV_RT][NB];
#pragma unroll
    for (int t = 0; t < RECV_RT; ++t)
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[t][j] = make_double2(0.0, 0.0);
    const int lines = g.m * g.l;
    for (int line = blockIdx.x * lp + lt; line < lines; line += gridDim.x * lp) {
        const int iz = line / g.m, iy = line - iz * g.m;
        cplx eyz[RECV_RT];
#pragma unroll
        for (int t = 0; t < RECV_RT; ++t) {
            eyz[t] = T[t][g.n + iy];
            if constexpr (DIM == 3) eyz[t] = cmul(eyz[t], T[t][g.n + g.m + iz]);
        }
        const int64_t base = (int64_t)line * g.n;
        for (int ix = xt; ix < g.n; ix += xstep) {
            const int64_t i = base + ix;
            cplx qv[NB];
#pragma unroll
            for (int j = 0; j < NB; ++j) qv[j] = q[(size_t)j * N + i];
            if (md.nu) {
                const cplx f = medium_factor(md, i, false);
#pragma unroll
                for (int j = 0; j < NB; ++j) qv[j] = medium_mul(md, f, qv[j]);
            }
#pragma unroll
            for (int t = 0; t < RECV_RT; ++t) {
                const cplx w = cmul(eyz[t], T[t][ix]);
#pragma unroll
                for (int j = 0; j < NB; ++j) cfma(acc[t][j], w, qv[j]);
            }
        }
    }
    store_partials<NB>(acc, r0, nrecv, rpass, partial);
}

// second stage: one wave per (receiver of the pass, member) adds the block partials in index order; far field: times c_d h^d
__global__ __launch_bounds__(64) void k_recv_finish(const cplx* __restrict__ partial, int blocks, int rpass, int scaled, double cre, double cim,
                                                    cplx* __restrict__ out, int64_t out_stride) {
    const cplx s = finish_in_wave(partial + ((size_t)blockIdx.y * rpass + blockIdx.x) * blocks, blocks);
    if (threadIdx.x == 0) out[(size_t)blockIdx.y * out_stride + blockIdx.x] = scaled ? cmul(make_double2(cre, cim), s) : s;
}

// T / H: out_j[i] = [scale nu_i] sum_r g(r, i) w_j[r] (T), the same with conj(g) and conj(nu) (H); r = 0 .. nrecv-1 in order
template <int DIM, int KIND, int NB> __global__ __launch_bounds__(256)
void k_recv_adj(Geo g, Medium md, int conj, double cre, double cim, const double* __restrict__ coords, const cplx* __restrict__ tab,
                int nrecv, const cplx* __restrict__ w, cplx* __restrict__ out, int64_t N) {
    __shared__ double sp[RECV_CHUNK * 3];
    __shared__ cplx sw[RECV_CHUNK][NB];
    const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = i0 < N;
    const int64_t i = live ? i0 : N - 1;                  // idle lanes of the last block compute the last point and store nothing
    int ix = (int)(i % g.n), iy = (int)((i / g.n) % g.m), iz = (int)(i / ((int64_t)g.n * g.m));
    if constexpr (DIM == 2) { iy = (int)(i / g.n); iz = 0; }
    const double x = fma(g.h, (double)ix, g.ox), y = fma(g.h, (double)iy, g.oy), z = DIM == 3 ? fma(g.h, (double)iz, g.oz) : 0.0;
    const int tl = g.n + g.m + g.l;
    cplx acc[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[j] = make_double2(0.0, 0.0);
    for (int c0 = 0; c0 < nrecv; c0 += RECV_CHUNK) {
        const int cnt = min(RECV_CHUNK, nrecv - c0);
        __syncthreads();                                  // the chunk before this one has been read by every wave
        if constexpr (KIND == LSFC_RECV_POINTS) for (int e = threadIdx.x; e < cnt * 3; e += 256) sp[e] = coords[(size_t)c0 * 3 + e];
        for (int e = threadIdx.x; e < cnt * NB; e += 256) { const int r = e / NB, j = e - r * NB; sw[r][j] = w[(size_t)j * nrecv + c0 + r]; }
        __syncthreads();
        for (int r = 0; r < cnt; ++r) {
            cplx gv;
            if constexpr (KIND == LSFC_RECV_POINTS) gv = green<DIM>(g, sp[3 * r] - x, sp[3 * r + 1] - y, sp[3 * r + 2] - z);
            else {
                const cplx* T = tab + (size_t)(c0 + r) * tl;
                gv = cmul(T[ix], T[g.n + iy]);
                if constexpr (DIM == 3) gv = cmul(gv, T[g.n + g.m + iz]);
            }
            if (conj) gv.y = -gv.y;
#pragma unroll
            for (int j = 0; j < NB; ++j) cfma(acc[j], gv, sw[r][j]);
        }
    }
    if (!live) return;
    const cplx f = md.nu ? medium_factor(md, i, conj != 0) : make_double2(0.0, 0.0);
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        cplx v = acc[j];
        if constexpr (KIND == LSFC_RECV_FARFIELD) v = cmul(make_double2(cre, conj ? -cim : cim), v);
        if (md.nu) v = medium_mul(md, f, v);
        out[(size_t)j * N + i] = v;
    }
}

__global__ void k_warmup_receivers(int* p) { if (p) *p = 0; }

Geo geo_of(const lsfc_receivers* rc) {
    const double h = rc->h, pi = 3.14159265358979323846;
    return Geo{rc->dims[0], rc->dims[1], rc->dims[2], rc->origin[0], rc->origin[1], rc->origin[2], h, rc->k,
               rc->ndim == 3 ? h * h * h / (4.0 * pi) : h * h / 4.0};
}
// c_d h^d of the far-field rows: h^3 / (4 pi), h^2 e^{i pi/4} / sqrt(8 pi k)
cplx far_constant(const lsfc_receivers* rc) {
    const double h = rc->h, pi = 3.14159265358979323846;
    if (rc->ndim == 3) return make_double2(h * h * h / (4.0 * pi), 0.0);
    const double a = h * h / std::sqrt(8.0 * pi * rc->k), s = std::sqrt(0.5);
    return make_double2(a * s, a * s);
}
Medium medium_of(const lsfc_plan* plan) {
    if (!plan) return Medium{nullptr, nullptr, 0.0};
    return Medium{plan->nu.p, plan->nu_im.p, -(plan->omega * plan->omega)};
}

// one group of cnt <= LSFC_MAX_BATCH members, device pointers, stream-ordered
void forward_group(lsfc_receivers* rc, const lsfc_plan* plan, const cplx* in, cplx* out, int cnt) {
    const Geo g = geo_of(rc);
    const Medium md = medium_of(plan);
    const int blocks = red_blocks(rc->N);
    const bool far = rc->kind == LSFC_RECV_FARFIELD;
    const cplx c = far ? far_constant(rc) : make_double2(1.0, 0.0);
    const int64_t S = (int64_t)blocks * RED_THREADS;
    const Stride st = rc->ndim == 3 ? Stride{(int)(S % g.n), (int)((S / g.n) % g.m), (int)(S / ((int64_t)g.n * g.m))} : Stride{(int)(S % g.n), (int)(S / g.n), 0};
    int xshift = 0;
    while ((1 << xshift) < g.n && xshift < 6) ++xshift;                      // up to one wave along a line of x
    const int tl = g.n + g.m + g.l;
    for (int64_t r0 = 0; r0 < rc->nrecv; r0 += RECV_PASS) {
        const int rp = (int)std::min<int64_t>(RECV_PASS, rc->nrecv - r0);
        const dim3 grid((unsigned)blocks, (unsigned)((rp + RECV_RT - 1) / RECV_RT));
        dispatch<1, LSFC_MAX_BATCH>(cnt, "lsfc_receivers_apply", [&](auto nb) {
            constexpr int NB = decltype(nb)::value;
            if (far) {
                auto kern = rc->ndim == 3 ? k_recv_fwd_far<3, NB> : k_recv_fwd_far<2, NB>;
                hipLaunchKernelGGL(kern, grid, dim3(RED_THREADS), 0, rc->stream, g, xshift, md, rc->tab.p + (size_t)r0 * tl, rp, rp, in, rc->N, rc->partial.p);
            } else {
                auto kern = rc->ndim == 3 ? k_recv_fwd_points<3, NB> : k_recv_fwd_points<2, NB>;
                hipLaunchKernelGGL(kern, grid, dim3(RED_THREADS), 0, rc->stream, g, st, md, rc->coords.p + (size_t)r0 * 3, rp, rp, in, rc->N, rc->partial.p);
            }
        });
        LSFC_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_recv_finish, dim3((unsigned)rp, (unsigned)cnt), dim3(64), 0, rc->stream, rc->partial.p, blocks, rp, far ? 1 : 0, c.x, c.y,
                           out + r0, rc->nrecv);
        LSFC_HIP(hipGetLastError());
    }
}

void adjoint_group(lsfc_receivers* rc, const lsfc_plan* plan, const cplx* in, cplx* out, int cnt, bool conj) {
    const Geo g = geo_of(rc);
    const Medium md = medium_of(plan);
    const bool far = rc->kind == LSFC_RECV_FARFIELD;
    const cplx c = far ? far_constant(rc) : make_double2(1.0, 0.0);
    const dim3 grid((unsigned)((rc->N + 255) / 256));
    dispatch<1, LSFC_MAX_BATCH>(cnt, "lsfc_receivers_apply", [&](auto nb) {
        constexpr int NB = decltype(nb)::value;
        auto kern = far ? (rc->ndim == 3 ? k_recv_adj<3, LSFC_RECV_FARFIELD, NB> : k_recv_adj<2, LSFC_RECV_FARFIELD, NB>)
                        : (rc->ndim == 3 ? k_recv_adj<3, LSFC_RECV_POINTS, NB> : k_recv_adj<2, LSFC_RECV_POINTS, NB>);
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, rc->stream, g, md, conj ? 1 : 0, c.x, c.y, rc->coords.p, rc->tab.p, (int)rc->nrecv, in, out, rc->N);
    });
    LSFC_HIP(hipGetLastError());
}

// nrhs members on the device, in groups of LSFC_MAX_BATCH
void apply_dev(lsfc_receivers* rc, const lsfc_plan* plan, const cplx* in, cplx* out, int64_t nrhs, int op) {
    const int64_t nin = op == LSFC_OP_N ? rc->N : rc->nrecv, nout = op == LSFC_OP_N ? rc->nrecv : rc->N;
    if (op == LSFC_OP_N) {
        const size_t need = (size_t)std::min<int64_t>(nrhs, LSFC_MAX_BATCH) * (size_t)std::min<int64_t>(rc->nrecv, RECV_PASS) * (size_t)red_blocks(rc->N);
        if (rc->partial.n < need) rc->partial.alloc(need);
    }
    for (int64_t j0 = 0; j0 < nrhs; j0 += LSFC_MAX_BATCH) {
        const int cnt = (int)std::min<int64_t>(LSFC_MAX_BATCH, nrhs - j0);
        if (op == LSFC_OP_N) forward_group(rc, plan, in + j0 * nin, out + j0 * nout, cnt);
        else adjoint_group(rc, plan, in + j0 * nin, out + j0 * nout, cnt, op == LSFC_OP_H);
    }
}

} // namespace

void warmup_receivers() {
    hipLaunchKernelGGL(k_warmup_receivers, dim3(1), dim3(64), 0, 0, (int*)nullptr);
    LSFC_HIP(hipGetLastError());
}

int receivers_device(const lsfc_receivers* rc) { return rc->device; }

} // namespace lsfc

using namespace lsfc;

extern "C" {

int lsfc_receivers_create(lsfc_receivers** out, int ndim, const int64_t dims[3], const double origin[3], double h, double k,
                          int kind, const double* coords, int64_t nrecv, int device) {
    return guarded([&] {
        LSFC_REQUIRE(out, "NULL argument"); *out = nullptr;
        LSFC_REQUIRE(dims && origin && coords, "NULL argument");
        LSFC_REQUIRE(ndim == 2 || ndim == 3, "receivers: ndim = %d (2 or 3)", ndim);
        int64_t N = 1;
        for (int a = 0; a < ndim; ++a) {
            LSFC_REQUIRE(dims[a] >= 1, "receivers: dimension %d is %lld (at least 1)", a, (long long)dims[a]);
            LSFC_REQUIRE(dims[a] < ((int64_t)1 << 31) && N * dims[a] < ((int64_t)1 << 31), "receivers: more than 2^31 - 1 grid points");
            N *= dims[a];
        }
        LSFC_REQUIRE(h > 0.0 && std::isfinite(h), "receivers: h = %g (must be positive)", h);
        LSFC_REQUIRE(k > 0.0 && std::isfinite(k), "receivers: k = %g (must be positive and real)", k);
        LSFC_REQUIRE(kind == LSFC_RECV_POINTS || kind == LSFC_RECV_FARFIELD, "receivers: unknown kind %d (LSFC_RECV_POINTS or LSFC_RECV_FARFIELD)", kind);
        LSFC_REQUIRE(nrecv >= 1 && nrecv < ((int64_t)1 << 31), "receivers: nrecv = %lld (at least 1)", (long long)nrecv);
        for (int64_t r = 0; r < nrecv; ++r) {
            const double* p = coords + r * ndim;
            for (int a = 0; a < ndim; ++a) LSFC_REQUIRE(std::isfinite(p[a]), "receivers: coordinate %d of receiver %lld is not finite", a, (long long)r);
            if (kind == LSFC_RECV_FARFIELD) {
                double s = 0.0;
                for (int a = 0; a < ndim; ++a) s += p[a] * p[a];
                LSFC_REQUIRE(std::fabs(std::sqrt(s) - 1.0) <= 1e-12, "receivers: far-field direction %lld has norm %.17g (a unit vector is needed)", (long long)r, std::sqrt(s));
            } else {
                // the nearest grid point, by rounding
                double d2 = 0.0;
                for (int a = 0; a < ndim; ++a) {
                    double t = std::nearbyint((p[a] - origin[a]) / h);
                    t = std::min(std::max(t, 0.0), (double)(dims[a] - 1));
                    const double d = p[a] - (origin[a] + h * t);
                    d2 += d * d;
                }
                LSFC_REQUIRE(std::sqrt(d2) >= 1e-8 * h, "receivers: point receiver %lld lies on a grid point (distance %.3g, below 1e-8 h): receivers on grid points are out of scope",
                             (long long)r, std::sqrt(d2));
            }
        }
        select_device(device, "receivers operator");
        pruned_warmup(device);
        std::unique_ptr<lsfc_receivers> rc(new lsfc_receivers());
        rc->device = device; rc->ndim = ndim; rc->kind = kind; rc->h = h; rc->k = k; rc->N = N; rc->nrecv = nrecv;
        for (int a = 0; a < ndim; ++a) { rc->dims[a] = (int)dims[a]; rc->origin[a] = origin[a]; }
        if (kind == LSFC_RECV_POINTS) {
            std::vector<double> c3((size_t)nrecv * 3, 0.0);
            for (int64_t r = 0; r < nrecv; ++r) for (int a = 0; a < ndim; ++a) c3[(size_t)(3 * r + a)] = coords[r * ndim + a];
            rc->coords.alloc(c3.size());
            LSFC_HIP(hipMemcpy(rc->coords.p, c3.data(), rc->coords.bytes(), hipMemcpyHostToDevice));
        } else {
            // every entry by its own sincos, no recurrences; the axes a direction does not have (2D: z) hold 1
            const int tl = rc->dims[0] + rc->dims[1] + rc->dims[2];
            std::vector<cplx> t((size_t)nrecv * tl);
            for (int64_t r = 0; r < nrecv; ++r) {
                cplx* row = t.data() + (size_t)r * tl;
                for (int a = 0; a < 3; ++a) {
                    const double th = a < ndim ? coords[r * ndim + a] : 0.0;
                    for (int i = 0; i < rc->dims[a]; ++i) {
                        const double ph = -k * th * (rc->origin[a] + h * (double)i);
                        *row++ = make_double2(std::cos(ph), std::sin(ph));
                    }
                }
            }
            rc->tab.alloc(t.size());
            LSFC_HIP(hipMemcpy(rc->tab.p, t.data(), rc->tab.bytes(), hipMemcpyHostToDevice));
        }
        *out = rc.release();
    });
}

int lsfc_receivers_destroy(lsfc_receivers* rc) {
    return guarded([&] { if (rc) { (void)hipSetDevice(rc->device); (void)hipDeviceSynchronize(); delete rc; } });
}

int lsfc_receivers_set_stream(lsfc_receivers* rc, void* hip_stream) {
    return guarded([&] { LSFC_REQUIRE(rc, "NULL receivers"); rc->stream = (hipStream_t)hip_stream; });
}

int lsfc_receivers_apply(lsfc_receivers* rc, lsfc_plan* plan, const double* in, double* out, int64_t nrhs, int op, int memspace) {
    return guarded([&] {
        LSFC_REQUIRE(rc && in && out, "NULL argument");
        LSFC_REQUIRE(nrhs >= 1 && nrhs < ((int64_t)1 << 31), "receivers: nrhs = %lld (at least 1)", (long long)nrhs);
        LSFC_REQUIRE(op == LSFC_OP_N || op == LSFC_OP_T || op == LSFC_OP_H, "receivers: bad op %d (LSFC_OP_N, LSFC_OP_T or LSFC_OP_H)", op);
        LSFC_REQUIRE(memspace == LSFC_MEM_HOST || memspace == LSFC_MEM_DEVICE, "receivers: bad memspace %d", memspace);
        if (plan) {
            LSFC_REQUIRE(!plan->multi, "the fused receivers apply is not available on a multi-device plan");
            LSFC_REQUIRE(!plan->dist, "the fused receivers apply is not available on a distributed (or simulated-rank) plan");
            LSFC_REQUIRE(plan->N == rc->N, "receivers: the plan has %lld grid points, the receivers object %lld", (long long)plan->N, (long long)rc->N);
            LSFC_REQUIRE(plan->device == rc->device, "receivers: the plan lives on device %d, the receivers object on device %d", plan->device, rc->device);
        }
        LSFC_HIP(hipSetDevice(rc->device));
        const int64_t nin = op == LSFC_OP_N ? rc->N : rc->nrecv, nout = op == LSFC_OP_N ? rc->nrecv : rc->N;
        if (memspace == LSFC_MEM_DEVICE) { apply_dev(rc, plan, (const cplx*)in, (cplx*)out, nrhs, op); return; }
        // host vectors: a group at a time through the staging buffers; synchronised on return
        const int64_t grp = std::min<int64_t>(nrhs, LSFC_MAX_BATCH);
        if (rc->hin.n < (size_t)(grp * nin)) rc->hin.alloc((size_t)(grp * nin));
        if (rc->hout.n < (size_t)(grp * nout)) rc->hout.alloc((size_t)(grp * nout));
        for (int64_t j0 = 0; j0 < nrhs; j0 += grp) {
            const int64_t cnt = std::min<int64_t>(grp, nrhs - j0);
            LSFC_HIP(hipMemcpyAsync(rc->hin.p, (const cplx*)in + j0 * nin, (size_t)(cnt * nin) * sizeof(cplx), hipMemcpyHostToDevice, rc->stream));
            apply_dev(rc, plan, rc->hin.p, rc->hout.p, cnt, op);
            LSFC_HIP(hipMemcpyAsync((cplx*)out + j0 * nout, rc->hout.p, (size_t)(cnt * nout) * sizeof(cplx), hipMemcpyDeviceToHost, rc->stream));
        }
        LSFC_HIP(hipStreamSynchronize(rc->stream));
    });
}

int lsfc_receivers_info(const lsfc_receivers* rc, int64_t out[6]) {
    return guarded([&] {
        LSFC_REQUIRE(rc && out, "NULL argument");
        out[0] = rc->N; out[1] = rc->nrecv; out[2] = RECV_RT; out[3] = RECV_CHUNK; out[4] = LSFC_MAX_BATCH;
        out[5] = (int64_t)(rc->coords.bytes() + rc->tab.bytes());
    });
}

} // extern "C"
