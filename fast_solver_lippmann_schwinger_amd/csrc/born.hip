// Linearised scattering (lsfc_born_*; DESIGN.md section 3, "Linearised scattering"): the Frechet derivative J of the map
// nu -> data d_s = -omega^2 R (nu .* u_s), M u_s = u_inc_s, its adjoint and so the gradient of a least-squares misfit.
//     J_s dnu = -omega^2 R M^-T (u_s .* dnu)                       one M^T solve per source, then the plain R
//     J^H r   = sum_s -omega^2 conj(u_s .* p_s),  M p_s = R^T conj(r_s)     one M solve per source (reciprocity)
// The solves are the library's lock-step batched solvers and R is the receivers object; what is new here are three streaming
// kernels and the object that puts them in sequence:
//     k_born_scale   out_j = dnu .* u_j for the members of a group; dnu is read once per group
//     k_born_image   g = [g +] sum_j scale conj(u_j .* p_j), serially in member order, so that a point's bits depend on the order
//                    of the sources and on nothing else (groups, chunks and launches continue from the running value in g)
//     k_conj_small   the conjugated residuals in front of R^T
// One 16-B access per complex, grid-stride loops over grid_for blocks, no atomics, no LDS, no host work inside a call.  conj(M)^-1
// is none of N / T / H, which is why the conjugations of J^H sit in these kernels and not in an op.
// Reciprocal mode (lsfc_born_set_mode): one solve per receiver and medium for V = M^-1 R^T, and since R M^-T = V^T both applies are
// contractions of the stored U and V without a solve (born_contract.hip); k_identity_rows makes the right-hand sides' e_r.
#include "plan.hpp"
#include "receivers.hpp"
#include "born_contract.hpp"
#include "reduce.hpp"
#include <algorithm>
#include <memory>
#include <vector>

struct lsfc_born {
    lsfc_plan* plan = nullptr;
    lsfc_receivers* rc = nullptr;
    lsfc_born_opts o{};
    int device = 0;
    int64_t N = 0, nrecv = 0, nsrc = 0, chunk = 0;
    lsfc::DevBuf<lsfc::cplx> U;        // the background fields, nsrc x N
    lsfc::DevBuf<lsfc::cplx> W;        // 2 chunk + 1 work vectors: right-hand sides, solutions, one vector of staging
    lsfc::DevBuf<lsfc::cplx> data;     // d_s at the receivers, nsrc x nrecv
    lsfc::DevBuf<lsfc::cplx> small;    // two vectors of nsrc x nrecv: staged residuals / data perturbations and conj(r)
    std::vector<lsfc_gmres_result> last;               // per source, of the last call
    int64_t last_solves = 0, last_mvps = 0, first_bad = -1;
    const char* bad_stage = "";
    // reciprocal mode (lsfc_born_set_mode): the receiver fields V = M^-1 R^T, nrecv x N, and the block partials of the contraction
    int mode = LSFC_BORN_ADJOINT_STATE;
    lsfc::DevBuf<lsfc::cplx> V;
    lsfc::DevBuf<double> cwork;
    bool have_v = false;
    std::vector<lsfc_gmres_result> recv_last;          // per receiver, of the last receiver-field solve
    int64_t recv_solves = 0, recv_mvps = 0, recv_bad = -1;
};

namespace lsfc {
namespace {

constexpr int BORN_THREADS = 256;

// out_j[i] = (factor dnu[i]) u_j[i]; out may be u (each thread reads a point of a member before it writes it)
template <int NB, bool CPLX> __global__ __launch_bounds__(BORN_THREADS)
void k_born_scale(const double* __restrict__ dnu, double factor, const cplx* u, cplx* out, int64_t N) {
    const int64_t step = (int64_t)gridDim.x * BORN_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * BORN_THREADS + threadIdx.x; i < N; i += step) {
        cplx d;
        if constexpr (CPLX) { d = reinterpret_cast<const cplx*>(dnu)[i]; d.x *= factor; d.y *= factor; }
        else d = make_double2(factor * dnu[i], 0.0);
        cplx v[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) v[j] = u[(size_t)j * N + i];
#pragma unroll
        for (int j = 0; j < NB; ++j) out[(size_t)j * N + i] = CPLX ? cprod(d, v[j]) : make_double2(d.x * v[j].x, d.x * v[j].y);
    }
}

// g[i] = (accumulate ? g[i] : 0) + sum_j scale conj(u_j[i] p_j[i]), j = 0 .. NB-1 in order.  REAL: g is N doubles and the sum is
// that of the real parts -- the real part of the running value never reads the imaginary one, so its bits are those of the
// complex form
template <int NB, bool REAL> __global__ __launch_bounds__(BORN_THREADS)
void k_born_image(const cplx* __restrict__ u, const cplx* __restrict__ p, cplx scale, int accumulate, double* g, int64_t N) {
    const int64_t step = (int64_t)gridDim.x * BORN_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * BORN_THREADS + threadIdx.x; i < N; i += step) {
        cplx acc = make_double2(0.0, 0.0);
        if (accumulate) { if constexpr (REAL) acc.x = g[i]; else acc = reinterpret_cast<const cplx*>(g)[i]; }
        cplx uv[NB], pv[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) { uv[j] = u[(size_t)j * N + i]; pv[j] = p[(size_t)j * N + i]; }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            cplx t = cprod(uv[j], pv[j]);
            t.y = -t.y;
            acc = caddmul(acc, scale, t);
        }
        if constexpr (REAL) g[i] = acc.x; else reinterpret_cast<cplx*>(g)[i] = acc;
    }
}

// rows r0 .. r0 + cnt - 1 of the nrecv x nrecv identity, in front of R^T
__global__ __launch_bounds__(BORN_THREADS) void k_identity_rows(cplx* __restrict__ out, int64_t r0, int64_t cnt, int64_t nrecv) {
    const int64_t step = (int64_t)gridDim.x * BORN_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * BORN_THREADS + threadIdx.x; i < cnt * nrecv; i += step)
        out[i] = make_double2(i % nrecv == r0 + i / nrecv ? 1.0 : 0.0, 0.0);
}

__global__ __launch_bounds__(BORN_THREADS) void k_conj_small(const cplx* __restrict__ in, cplx* __restrict__ out, int64_t n) {
    const int64_t step = (int64_t)gridDim.x * BORN_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * BORN_THREADS + threadIdx.x; i < n; i += step) { const cplx v = in[i]; out[i] = make_double2(v.x, -v.y); }
}

// nrhs members back to back on the device, in groups of LSFC_MAX_BATCH; stream-ordered
void scale_dev(hipStream_t st, const double* dnu, bool is_complex, double factor, const cplx* u, cplx* out, int64_t nrhs, int64_t N) {
    for (int64_t j0 = 0; j0 < nrhs; j0 += LSFC_MAX_BATCH) {
        const int cnt = (int)std::min<int64_t>(LSFC_MAX_BATCH, nrhs - j0);
        dispatch<1, LSFC_MAX_BATCH>(cnt, "lsfc_born_scale", [&](auto nb) {
            constexpr int NB = decltype(nb)::value;
            auto kern = is_complex ? k_born_scale<NB, true> : k_born_scale<NB, false>;
            hipLaunchKernelGGL(kern, dim3(grid_for(N, BORN_THREADS)), dim3(BORN_THREADS), 0, st, dnu, factor, u + j0 * N, out + j0 * N, N);
        });
        LSFC_HIP(hipGetLastError());
    }
}

void image_dev(hipStream_t st, const cplx* u, const cplx* p, int64_t nrhs, cplx scale, bool accumulate, bool real, double* g, int64_t N) {
    for (int64_t j0 = 0; j0 < nrhs; j0 += LSFC_MAX_BATCH) {
        const int cnt = (int)std::min<int64_t>(LSFC_MAX_BATCH, nrhs - j0);
        dispatch<1, LSFC_MAX_BATCH>(cnt, "lsfc_born_image", [&](auto nb) {
            constexpr int NB = decltype(nb)::value;
            auto kern = real ? k_born_image<NB, true> : k_born_image<NB, false>;
            hipLaunchKernelGGL(kern, dim3(grid_for(N, BORN_THREADS)), dim3(BORN_THREADS), 0, st, u + j0 * N, p + j0 * N, scale, (accumulate || j0 > 0) ? 1 : 0, g, N);
        });
        LSFC_HIP(hipGetLastError());
    }
}

void require_single_device(const lsfc_plan* plan, const char* who) {
    LSFC_REQUIRE(!plan->multi, "%s is not available on a multi-device plan", who);
    LSFC_REQUIRE(!plan->dist, "%s is not available on a distributed (or simulated-rank) plan", who);
}

// passes the error of a nested C ABI call on, under `who`
void nested(int rc, const char* who) {
    if (rc != LSFC_OK) { const std::string msg = lsfc_last_error(); fail(rc, "%s: %s", who, msg.c_str()); }
}

// The plan and the preconditioner mean `op` while this lives, and what they meant before afterwards, on every way out.  The
// preconditioner goes first: if it cannot follow (an object of lsfc_precond_create under T), nothing has changed yet.
struct OpGuard {
    lsfc_plan* plan; lsfc_precond* pc; int plan_op, pc_op = LSFC_OP_N;
    OpGuard(lsfc_born* b, int op, const char* who) : plan(b->plan), pc(b->o.precond), plan_op(b->plan->op) {
        if (pc) {
            nested(lsfc_precond_get_op(pc, &pc_op, nullptr), who);
            if (pc_op != op) {
                const int rc = lsfc_precond_set_op(pc, op);
                if (rc != LSFC_OK) {
                    const std::string msg = lsfc_last_error();
                    fail(rc, "%s: the solves of this call run on %s and the preconditioner cannot follow: %s", who, op == LSFC_OP_T ? "M^T" : "M", msg.c_str());
                }
            }
        }
        if (plan_op != op) {
            const int rc = lsfc_plan_set_op(plan, op);
            if (rc != LSFC_OK) { const std::string msg = lsfc_last_error(); restore(); fail(rc, "%s: %s", who, msg.c_str()); }
        }
    }
    void restore() { plan->op = plan_op; if (pc) (void)lsfc_precond_set_op(pc, pc_op); }
    ~OpGuard() { restore(); }
};

int restart_of(const lsfc_born* b) { return b->o.restart > 0 ? b->o.restart : (int)std::min<int64_t>(20, b->N); }
// work vectors of the solver per member: the rules of lsfc_gmres_batch and lsfc_bicgstabl_batch
int solver_vectors(const lsfc_born* b) { return b->o.solver == LSFC_BORN_GMRES ? restart_of(b) + 2 : 2 * b->o.l + 3; }

// cnt <= chunk solves in lock step, x0 = 0, under the op the plan has now; res: the results of members s0 .. s0 + cnt - 1, counted
// into solves / mvps / first_bad
void solve_members(lsfc_born* b, const cplx* rhs, cplx* x, int64_t s0, int cnt, const char* stage, lsfc_gmres_result* res,
                   int64_t& solves, int64_t& mvps, int64_t& first_bad) {
    lsfc_plan* p = b->plan;
    LSFC_HIP(hipMemsetAsync(x, 0, (size_t)cnt * (size_t)b->N * sizeof(cplx), p->stream));
    lsfc_precond_fn fn = b->o.precond ? &lsfc_precond_callback : nullptr;
    int rc;
    if (b->o.solver == LSFC_BORN_GMRES) {
        lsfc_gmres_opts g{};
        g.restart = b->o.restart; g.maxiter = b->o.maxiter; g.reltol = b->o.reltol; g.abstol = b->o.abstol;
        g.orth = LSFC_ORTH_MGS; g.initially_zero = 1;
        g.precond = fn; g.precond_user = b->o.precond; g.precond_on_device = fn ? 1 : 0;
        rc = lsfc_gmres_batch(p, (double*)x, (const double*)rhs, cnt, &g, nullptr, 0, res, LSFC_MEM_DEVICE);
    } else {
        lsfc_bicgstabl_opts s{};
        s.l = b->o.l; s.max_mv_products = b->o.maxiter; s.reltol = b->o.reltol; s.abstol = b->o.abstol; s.initially_zero = 1;
        s.precond = fn; s.precond_user = b->o.precond; s.precond_on_device = fn ? 1 : 0;
        rc = lsfc_bicgstabl_batch(p, (double*)x, (const double*)rhs, cnt, &s, nullptr, 0, res, nullptr, LSFC_MEM_DEVICE);
    }
    nested(rc, stage);
    ++solves;
    for (int j = 0; j < cnt; ++j) {
        mvps += res[j].mvps;
        if (!res[j].converged && first_bad < 0) first_bad = s0 + j;
    }
}

// the solves of the sources s0 .. s0 + cnt - 1
void solve_chunk(lsfc_born* b, const cplx* rhs, cplx* x, int64_t s0, int cnt, const char* stage) {
    const int64_t bad = b->first_bad;
    solve_members(b, rhs, x, s0, cnt, stage, b->last.data() + s0, b->last_solves, b->last_mvps, b->first_bad);
    if (bad < 0 && b->first_bad >= 0) b->bad_stage = stage;
}

// preconditioner and receivers run on the plan's stream
void bind_streams(lsfc_born* b) {
    LSFC_HIP(hipSetDevice(b->plan->device));
    if (b->o.precond) nested(lsfc_precond_set_stream(b->o.precond, b->plan->stream), "lsfc_born");
    nested(lsfc_receivers_set_stream(b->rc, b->plan->stream), "lsfc_born");
}

void begin_call(lsfc_born* b) {
    b->last_solves = b->last_mvps = 0; b->first_bad = -1; b->bad_stage = "";
    for (auto& r : b->last) r = lsfc_gmres_result{};
    bind_streams(b);
}

constexpr const char* RECEIVER_STAGE = "receiver-field solve on M";

// bytes that reciprocal mode holds beside the rest: V and the block partials of the contraction
double reciprocal_bytes(const lsfc_born* b, int64_t nsrc) {
    return (double)b->nrecv * (double)b->N * sizeof(cplx) + (double)contract_n_work(b->N, nsrc, b->nrecv) * sizeof(double);
}

// V = M^-1 R^T, `chunk` receivers at a time: rows of the identity through R^T, then the object's solver on M with x0 = 0.  U, W and
// small are allocated; V and cwork are allocated here.  A receiver that does not converge does not stop the others.
void solve_receiver_fields(lsfc_born* b, const char* who) {
    lsfc_plan* p = b->plan;
    const int64_t N = b->N, nrecv = b->nrecv;
    b->have_v = false;
    b->recv_solves = b->recv_mvps = 0; b->recv_bad = -1;
    b->recv_last.assign((size_t)nrecv, lsfc_gmres_result{});
    if (!b->V.p) b->V.alloc((size_t)(nrecv * N));
    b->cwork.alloc(contract_n_work(N, b->nsrc, nrecv));
    const OpGuard guard(b, LSFC_OP_N, who);
    cplx *rhs = b->W.p, *eye = b->small.p;
    for (int64_t r0 = 0; r0 < nrecv; r0 += b->chunk) {
        const int cnt = (int)std::min<int64_t>(b->chunk, nrecv - r0);
        hipLaunchKernelGGL(k_identity_rows, dim3(grid_for(cnt * nrecv, BORN_THREADS)), dim3(BORN_THREADS), 0, p->stream, eye, r0, (int64_t)cnt, nrecv);
        LSFC_HIP(hipGetLastError());
        nested(lsfc_receivers_apply(b->rc, nullptr, (const double*)eye, (double*)rhs, cnt, LSFC_OP_T, LSFC_MEM_DEVICE), who);
        solve_members(b, rhs, b->V.p + r0 * N, r0, cnt, RECEIVER_STAGE, b->recv_last.data() + r0, b->recv_solves, b->recv_mvps, b->recv_bad);
    }
    LSFC_HIP(hipStreamSynchronize(p->stream));
    b->have_v = true;
}

// LSFC_ENOTCONV after a call whose outputs are written: the first source that did not converge, and where; with `receivers`, after
// the sources, the first receiver of the receiver-field solve
int not_converged(const lsfc_born* b, int rc, const char* who, bool receivers = false) {
    if (rc == LSFC_OK && b->first_bad < 0 && receivers && b->recv_bad >= 0) {
        const lsfc_gmres_result& r = b->recv_last[(size_t)b->recv_bad];
        set_last_error("%s: receiver %lld did not converge in the %s (%lld iterations, %lld operator applications, residual %.3e); the receiver "
                       "fields are kept, lsfc_born_receiver_info has every receiver's result", who, (long long)b->recv_bad, RECEIVER_STAGE,
                       (long long)r.iters, (long long)r.mvps, r.final_resnorm);
        return LSFC_ENOTCONV;
    }
    if (rc != LSFC_OK || b->first_bad < 0) return rc;
    const lsfc_gmres_result& r = b->last[(size_t)b->first_bad];
    char also[160] = "";
    if (receivers && b->recv_bad >= 0)
        snprintf(also, sizeof also, "; receiver %lld did not converge in the %s (lsfc_born_receiver_info)", (long long)b->recv_bad, RECEIVER_STAGE);
    set_last_error("%s: source %lld did not converge in the %s (%lld iterations, %lld operator applications, residual %.3e); the outputs are written, "
                   "lsfc_born_info has every source's result%s", who, (long long)b->first_bad, b->bad_stage, (long long)r.iters, (long long)r.mvps, r.final_resnorm, also);
    return LSFC_ENOTCONV;
}

} // namespace
} // namespace lsfc

using namespace lsfc;

extern "C" {

int lsfc_born_scale(lsfc_plan* plan, const double* dnu, int dnu_is_complex, const double* u, double* out, int64_t nrhs, int memspace) {
    return guarded([&] {
        LSFC_REQUIRE(plan && dnu && u && out, "lsfc_born_scale: NULL argument");
        LSFC_REQUIRE(dnu_is_complex == 0 || dnu_is_complex == 1, "lsfc_born_scale: dnu_is_complex = %d (0 or 1)", dnu_is_complex);
        LSFC_REQUIRE(nrhs >= 1 && nrhs < ((int64_t)1 << 31), "lsfc_born_scale: nrhs = %lld (at least 1)", (long long)nrhs);
        LSFC_REQUIRE(memspace == LSFC_MEM_HOST || memspace == LSFC_MEM_DEVICE, "lsfc_born_scale: bad memspace %d", memspace);
        require_single_device(plan, "lsfc_born_scale");
        LSFC_HIP(hipSetDevice(plan->device));
        const int64_t N = plan->N;
        if (memspace == LSFC_MEM_DEVICE) { scale_dev(plan->stream, dnu, dnu_is_complex != 0, 1.0, (const cplx*)u, (cplx*)out, nrhs, N); return; }
        DevBuf<double> dd; DevBuf<cplx> du;
        dd.alloc((size_t)N * (dnu_is_complex ? 2 : 1)); du.alloc((size_t)(nrhs * N));
        LSFC_HIP(hipMemcpyAsync(dd.p, dnu, dd.bytes(), hipMemcpyHostToDevice, plan->stream));
        LSFC_HIP(hipMemcpyAsync(du.p, u, du.bytes(), hipMemcpyHostToDevice, plan->stream));
        scale_dev(plan->stream, dd.p, dnu_is_complex != 0, 1.0, du.p, du.p, nrhs, N);
        LSFC_HIP(hipMemcpyAsync(out, du.p, du.bytes(), hipMemcpyDeviceToHost, plan->stream));
        LSFC_HIP(hipStreamSynchronize(plan->stream));
    });
}

int lsfc_born_image(lsfc_plan* plan, const double* u, const double* p, int64_t nrhs, double scale_re, double scale_im, unsigned flags,
                    double* g, int memspace) {
    return guarded([&] {
        LSFC_REQUIRE(plan && u && p && g, "lsfc_born_image: NULL argument");
        LSFC_REQUIRE(nrhs >= 1 && nrhs < ((int64_t)1 << 31), "lsfc_born_image: nrhs = %lld (at least 1)", (long long)nrhs);
        LSFC_REQUIRE((flags & ~(LSFC_BORN_ACCUMULATE | LSFC_BORN_REAL)) == 0, "lsfc_born_image: unknown flag in 0x%x (LSFC_BORN_ACCUMULATE | LSFC_BORN_REAL)", flags);
        LSFC_REQUIRE(memspace == LSFC_MEM_HOST || memspace == LSFC_MEM_DEVICE, "lsfc_born_image: bad memspace %d", memspace);
        require_single_device(plan, "lsfc_born_image");
        LSFC_HIP(hipSetDevice(plan->device));
        const int64_t N = plan->N;
        const bool real = (flags & LSFC_BORN_REAL) != 0, acc = (flags & LSFC_BORN_ACCUMULATE) != 0;
        const cplx scale = make_double2(scale_re, scale_im);
        if (memspace == LSFC_MEM_DEVICE) { image_dev(plan->stream, (const cplx*)u, (const cplx*)p, nrhs, scale, acc, real, g, N); return; }
        DevBuf<cplx> du, dp; DevBuf<double> dg;
        du.alloc((size_t)(nrhs * N)); dp.alloc((size_t)(nrhs * N)); dg.alloc((size_t)N * (real ? 1 : 2));
        LSFC_HIP(hipMemcpyAsync(du.p, u, du.bytes(), hipMemcpyHostToDevice, plan->stream));
        LSFC_HIP(hipMemcpyAsync(dp.p, p, dp.bytes(), hipMemcpyHostToDevice, plan->stream));
        if (acc) LSFC_HIP(hipMemcpyAsync(dg.p, g, dg.bytes(), hipMemcpyHostToDevice, plan->stream));
        image_dev(plan->stream, du.p, dp.p, nrhs, scale, acc, real, dg.p, N);
        LSFC_HIP(hipMemcpyAsync(g, dg.p, dg.bytes(), hipMemcpyDeviceToHost, plan->stream));
        LSFC_HIP(hipStreamSynchronize(plan->stream));
    });
}

int lsfc_born_create(lsfc_born** out, lsfc_plan* plan, lsfc_receivers* rc, const lsfc_born_opts* opts) {
    return guarded([&] {
        LSFC_REQUIRE(out, "lsfc_born_create: NULL argument"); *out = nullptr;
        LSFC_REQUIRE(plan && rc && opts, "lsfc_born_create: NULL argument");
        for (int i = 0; i < 6; ++i) LSFC_REQUIRE(opts->reserved[i] == 0, "lsfc_born_create: reserved[%d] = %d must be zero", i, opts->reserved[i]);
        LSFC_REQUIRE(opts->solver == LSFC_BORN_GMRES || opts->solver == LSFC_BORN_BICGSTABL, "lsfc_born_create: unknown solver %d (LSFC_BORN_GMRES or LSFC_BORN_BICGSTABL)", opts->solver);
        if (opts->solver == LSFC_BORN_BICGSTABL) LSFC_REQUIRE(opts->l >= 1 && opts->l <= 8, "lsfc_born_create: l = %d is outside 1..8", opts->l);
        LSFC_REQUIRE(opts->chunk <= KRYLOV_NRHS_MAX, "lsfc_born_create: chunk = %lld (at most %d sources are solved in lock step)", (long long)opts->chunk, KRYLOV_NRHS_MAX);
        require_single_device(plan, "the Born operator");
        int64_t info[6];
        nested(lsfc_receivers_info(rc, info), "lsfc_born_create");
        LSFC_REQUIRE(info[0] == plan->N, "lsfc_born_create: the plan has %lld grid points, the receivers object %lld", (long long)plan->N, (long long)info[0]);
        LSFC_REQUIRE(receivers_device(rc) == plan->device, "lsfc_born_create: the plan lives on device %d, the receivers object on device %d", plan->device, receivers_device(rc));
        LSFC_HIP(hipSetDevice(plan->device));
        // J needs M^T = I + w^2 diag(nu) G: the symmetry check of lsfc_plan_set_op, its message passed on; the op stays what it is
        const int op = plan->op;
        const int src = lsfc_plan_set_op(plan, LSFC_OP_T);
        plan->op = op;
        nested(src, "lsfc_born_create");
        std::unique_ptr<lsfc_born> b(new lsfc_born());
        b->plan = plan; b->rc = rc; b->o = *opts; b->device = plan->device; b->N = plan->N; b->nrecv = info[1];
        *out = b.release();
    });
}

int lsfc_born_destroy(lsfc_born* b) {
    return guarded([&] { if (b) { (void)hipSetDevice(b->device); (void)hipDeviceSynchronize(); delete b; } });
}

int lsfc_born_set_background(lsfc_born* b, const double* u_inc, int64_t nsrc, int memspace) {
    const int rc = guarded([&] {
        LSFC_REQUIRE(b && u_inc, "lsfc_born_set_background: NULL argument");
        LSFC_REQUIRE(nsrc >= 1 && nsrc < ((int64_t)1 << 31), "lsfc_born_set_background: nsrc = %lld (at least 1)", (long long)nsrc);
        LSFC_REQUIRE(memspace == LSFC_MEM_HOST || memspace == LSFC_MEM_DEVICE, "lsfc_born_set_background: bad memspace %d", memspace);
        const int64_t N = b->N;
        lsfc_plan* p = b->plan;
        LSFC_HIP(hipSetDevice(p->device));
        LSFC_HIP(hipStreamSynchronize(p->stream));
        b->nsrc = 0;
        b->U.release(); b->W.release(); b->data.release(); b->small.release(); b->V.release(); b->cwork.release();
        b->have_v = false;
        const bool recip = b->mode == LSFC_BORN_RECIPROCAL;
        // the memory rule, before anything is allocated: U, per member of a chunk the solver's vectors and two work vectors, one more
        {
            size_t free_b = 0, total_b = 0;
            LSFC_HIP(hipMemGetInfo(&free_b, &total_b));
            const double vec = (double)N * sizeof(cplx), per = ((double)solver_vectors(b) + 2.0) * vec;
            const double fixed = ((double)nsrc + 1.0) * vec + (recip ? reciprocal_bytes(b, nsrc) : 0.0);
            const int64_t cap = std::min<int64_t>(nsrc, KRYLOV_NRHS_MAX);
            const int64_t fit = (double)free_b > fixed ? (int64_t)(((double)free_b - fixed) / per) : 0;
            const int64_t chunk = b->o.chunk > 0 ? std::min<int64_t>(b->o.chunk, nsrc) : std::min(cap, fit);
            const double need = fixed + (double)std::max<int64_t>(chunk, 1) * per;
            if (chunk < 1 || need > (double)free_b) {
                const int64_t c1 = std::max<int64_t>(chunk, 1);
                const double left = (double)free_b - (double)c1 * per - vec;
                if (recip)
                    fail(LSFC_ENOMEM, "lsfc_born_set_background: %lld sources x %lld complex (U), %lld receiver fields (V, reciprocal mode) with the contraction's "
                         "work space, chunk %lld x (%d solver + 2 work) vectors and one more need %.2f GB of device memory, %.2f GB are free -- the largest "
                         "nrecv that fits with %lld sources at chunk %lld is about %lld",
                         (long long)nsrc, (long long)N, (long long)b->nrecv, (long long)c1, solver_vectors(b), need / 1e9, (double)free_b / 1e9, (long long)nsrc,
                         (long long)c1, (long long)std::max(0.0, (left - (double)nsrc * vec) / (vec * 1.01)));
                fail(LSFC_ENOMEM, "lsfc_born_set_background: %lld sources x %lld complex (U), chunk %lld x (%d solver + 2 work) vectors and one more need %.2f GB of device "
                     "memory, %.2f GB are free -- the largest chunk that fits with %lld sources is %lld, the largest nsrc at chunk %lld is %lld",
                     (long long)nsrc, (long long)N, (long long)c1, solver_vectors(b), need / 1e9, (double)free_b / 1e9, (long long)nsrc, (long long)std::min(cap, fit),
                     (long long)c1, (long long)(left > 0 ? left / vec : 0));
            }
            b->chunk = chunk;
        }
        b->U.alloc((size_t)(nsrc * N)); b->W.alloc((size_t)((2 * b->chunk + 1) * N));
        b->data.alloc((size_t)(nsrc * b->nrecv)); b->small.alloc((size_t)(2 * nsrc * b->nrecv));
        b->last.assign((size_t)nsrc, lsfc_gmres_result{});
        begin_call(b);
        {
            const OpGuard guard(b, LSFC_OP_N, "lsfc_born_set_background");
            for (int64_t s0 = 0; s0 < nsrc; s0 += b->chunk) {
                const int cnt = (int)std::min<int64_t>(b->chunk, nsrc - s0);
                const cplx* rhs = (const cplx*)u_inc + s0 * N;
                if (memspace == LSFC_MEM_HOST) {
                    LSFC_HIP(hipMemcpyAsync(b->W.p, rhs, (size_t)cnt * (size_t)N * sizeof(cplx), hipMemcpyHostToDevice, p->stream));
                    rhs = b->W.p;
                }
                solve_chunk(b, rhs, b->U.p + s0 * N, s0, cnt, "background solve on M");
            }
        }
        nested(lsfc_receivers_apply(b->rc, p, (const double*)b->U.p, (double*)b->data.p, nsrc, LSFC_OP_N, LSFC_MEM_DEVICE), "lsfc_born_set_background");
        LSFC_HIP(hipStreamSynchronize(p->stream));
        b->nsrc = nsrc;
        if (recip) solve_receiver_fields(b, "lsfc_born_set_background");
    });
    return b ? not_converged(b, rc, "lsfc_born_set_background", true) : rc;
}

int lsfc_born_fields(const lsfc_born* b, const double** u_dev, int64_t* nsrc) {
    return guarded([&] {
        LSFC_REQUIRE(b && u_dev && nsrc, "lsfc_born_fields: NULL argument");
        LSFC_REQUIRE(b->nsrc > 0, "lsfc_born_fields before lsfc_born_set_background");
        *u_dev = (const double*)b->U.p; *nsrc = b->nsrc;
    });
}

int lsfc_born_data(lsfc_born* b, double* d, int memspace) {
    return guarded([&] {
        LSFC_REQUIRE(b && d, "lsfc_born_data: NULL argument");
        LSFC_REQUIRE(memspace == LSFC_MEM_HOST || memspace == LSFC_MEM_DEVICE, "lsfc_born_data: bad memspace %d", memspace);
        LSFC_REQUIRE(b->nsrc > 0, "lsfc_born_data before lsfc_born_set_background");
        LSFC_HIP(hipSetDevice(b->plan->device));
        LSFC_HIP(hipMemcpyAsync(d, b->data.p, b->data.bytes(), memspace == LSFC_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, b->plan->stream));
        if (memspace == LSFC_MEM_HOST) LSFC_HIP(hipStreamSynchronize(b->plan->stream));
    });
}

int lsfc_born_apply(lsfc_born* b, const double* in, int in_is_complex, double* out, int op, unsigned flags, int memspace) {
    const bool reached = b && in && out;            // (whether b may be read after the call: the checks below come before it is)
    bool entered = false;
    const int rc = guarded([&] {
        LSFC_REQUIRE(b && in && out, "lsfc_born_apply: NULL argument");
        LSFC_REQUIRE(op == LSFC_OP_N || op == LSFC_OP_T || op == LSFC_OP_H, "lsfc_born_apply: bad op %d (LSFC_OP_N or LSFC_OP_H)", op);
        LSFC_REQUIRE(op != LSFC_OP_T, "lsfc_born_apply: LSFC_OP_T is not offered (J^T r = conj(J^H conj(r)) for the caller who needs it)");
        LSFC_REQUIRE((flags & ~LSFC_BORN_REAL) == 0, "lsfc_born_apply: unknown flag in 0x%x (LSFC_BORN_REAL)", flags);
        LSFC_REQUIRE(!(flags & LSFC_BORN_REAL) || op == LSFC_OP_H, "lsfc_born_apply: LSFC_BORN_REAL goes with LSFC_OP_H (the real part of the gradient), not with LSFC_OP_N");
        LSFC_REQUIRE(in_is_complex == 0 || in_is_complex == 1, "lsfc_born_apply: in_is_complex = %d (0 or 1)", in_is_complex);
        LSFC_REQUIRE(op == LSFC_OP_N || in_is_complex == 1, "lsfc_born_apply: the residuals of LSFC_OP_H are complex (in_is_complex = 1)");
        LSFC_REQUIRE(memspace == LSFC_MEM_HOST || memspace == LSFC_MEM_DEVICE, "lsfc_born_apply: bad memspace %d", memspace);
        LSFC_REQUIRE(b->nsrc > 0, "lsfc_born_apply before lsfc_born_set_background");
        entered = true;
        lsfc_plan* p = b->plan;
        const int64_t N = b->N, nsrc = b->nsrc, nd = nsrc * b->nrecv;
        const bool host = memspace == LSFC_MEM_HOST, real = (flags & LSFC_BORN_REAL) != 0;
        const double w2 = p->omega * p->omega;
        if (b->mode == LSFC_BORN_RECIPROCAL) {
            // no solves, no OpGuard: two contractions of the stored U and V
            LSFC_REQUIRE(b->have_v, "lsfc_born_apply: reciprocal mode without receiver fields (the receiver-field solve failed: lsfc_born_set_mode or lsfc_born_set_background again)");
            b->last_solves = b->last_mvps = 0; b->first_bad = -1; b->bad_stage = "";
            for (auto& r : b->last) { r = lsfc_gmres_result{}; r.converged = 1; }
            LSFC_HIP(hipSetDevice(p->device));
            cplx* stage = b->W.p + 2 * b->chunk * N;
            const cplx scale = make_double2(-w2, 0.0);
            if (op == LSFC_OP_N) {
                const double* dnu = in;
                if (host) {
                    LSFC_HIP(hipMemcpyAsync(stage, in, (size_t)N * (in_is_complex ? 16 : 8), hipMemcpyHostToDevice, p->stream));
                    dnu = (const double*)stage;
                }
                cplx* dd = host ? b->small.p : (cplx*)out;
                contract_n_dev(p->stream, b->U.p, nsrc, b->V.p, b->nrecv, dnu, in_is_complex != 0, dd, scale, N, b->cwork.p);
                if (host) LSFC_HIP(hipMemcpyAsync(out, dd, (size_t)nd * sizeof(cplx), hipMemcpyDeviceToHost, p->stream));
            } else {
                const cplx* r = (const cplx*)in;
                if (host) { LSFC_HIP(hipMemcpyAsync(b->small.p, in, (size_t)nd * sizeof(cplx), hipMemcpyHostToDevice, p->stream)); r = b->small.p; }
                double* g = host ? (double*)stage : out;
                contract_h_dev(p->stream, b->U.p, nsrc, b->V.p, b->nrecv, r, g, scale, false, real, N);
                if (host) LSFC_HIP(hipMemcpyAsync(out, g, (size_t)N * (real ? 8 : 16), hipMemcpyDeviceToHost, p->stream));
            }
            if (host) LSFC_HIP(hipStreamSynchronize(p->stream));
            return;
        }
        cplx *B = b->W.p, *X = b->W.p + b->chunk * N, *stage = b->W.p + 2 * b->chunk * N, *s0buf = b->small.p, *s1buf = b->small.p + nd;
        begin_call(b);
        const OpGuard guard(b, op == LSFC_OP_N ? LSFC_OP_T : LSFC_OP_N, "lsfc_born_apply");
        if (op == LSFC_OP_N) {
            const double* dnu = in;
            if (host) {
                LSFC_HIP(hipMemcpyAsync(stage, in, (size_t)N * (in_is_complex ? 16 : 8), hipMemcpyHostToDevice, p->stream));
                dnu = (const double*)stage;
            }
            cplx* dd = host ? s0buf : (cplx*)out;
            for (int64_t c0 = 0; c0 < nsrc; c0 += b->chunk) {
                const int cnt = (int)std::min<int64_t>(b->chunk, nsrc - c0);
                scale_dev(p->stream, dnu, in_is_complex != 0, -w2, b->U.p + c0 * N, B, cnt, N);
                solve_chunk(b, B, X, c0, cnt, "solve on M^T");
                nested(lsfc_receivers_apply(b->rc, nullptr, (const double*)X, (double*)(dd + c0 * b->nrecv), cnt, LSFC_OP_N, LSFC_MEM_DEVICE), "lsfc_born_apply");
            }
            if (host) LSFC_HIP(hipMemcpyAsync(out, dd, (size_t)nd * sizeof(cplx), hipMemcpyDeviceToHost, p->stream));
        } else {
            const cplx* r = (const cplx*)in;
            if (host) { LSFC_HIP(hipMemcpyAsync(s0buf, in, (size_t)nd * sizeof(cplx), hipMemcpyHostToDevice, p->stream)); r = s0buf; }
            hipLaunchKernelGGL(k_conj_small, dim3(grid_for(nd, BORN_THREADS)), dim3(BORN_THREADS), 0, p->stream, r, s1buf, nd);
            LSFC_HIP(hipGetLastError());
            double* g = host ? (double*)stage : out;
            for (int64_t c0 = 0; c0 < nsrc; c0 += b->chunk) {
                const int cnt = (int)std::min<int64_t>(b->chunk, nsrc - c0);
                nested(lsfc_receivers_apply(b->rc, nullptr, (const double*)(s1buf + c0 * b->nrecv), (double*)B, cnt, LSFC_OP_T, LSFC_MEM_DEVICE), "lsfc_born_apply");
                solve_chunk(b, B, X, c0, cnt, "adjoint-state solve on M");
                image_dev(p->stream, b->U.p + c0 * N, X, cnt, make_double2(-w2, 0.0), c0 > 0, real, g, N);
            }
            if (host) LSFC_HIP(hipMemcpyAsync(out, g, (size_t)N * (real ? 8 : 16), hipMemcpyDeviceToHost, p->stream));
        }
        if (host) LSFC_HIP(hipStreamSynchronize(p->stream));
    });
    return reached && entered ? not_converged(b, rc, "lsfc_born_apply") : rc;
}

int lsfc_born_info(const lsfc_born* b, int64_t out[8], lsfc_gmres_result* last) {
    return guarded([&] {
        LSFC_REQUIRE(b && out, "lsfc_born_info: NULL argument");
        out[0] = b->N; out[1] = b->nrecv; out[2] = b->nsrc; out[3] = b->chunk; out[4] = b->o.solver;
        out[5] = (int64_t)(b->U.bytes() + b->W.bytes() + b->data.bytes() + b->small.bytes() + b->V.bytes() + b->cwork.bytes());
        out[6] = b->last_solves; out[7] = b->last_mvps;
        if (last) for (int64_t s = 0; s < b->nsrc; ++s) last[s] = b->last[(size_t)s];
    });
}

int lsfc_born_set_mode(lsfc_born* b, int mode) {
    bool solved = false;
    const int rc = guarded([&] {
        LSFC_REQUIRE(mode == LSFC_BORN_ADJOINT_STATE || mode == LSFC_BORN_RECIPROCAL,
                     "lsfc_born_set_mode: unknown mode %d (LSFC_BORN_ADJOINT_STATE or LSFC_BORN_RECIPROCAL)", mode);
        LSFC_REQUIRE(b, "lsfc_born_set_mode: NULL argument");
        if (mode == b->mode && (mode == LSFC_BORN_ADJOINT_STATE || b->have_v || b->nsrc == 0)) return;
        LSFC_HIP(hipSetDevice(b->plan->device));
        LSFC_HIP(hipStreamSynchronize(b->plan->stream));
        if (mode == LSFC_BORN_ADJOINT_STATE) {
            b->V.release(); b->cwork.release(); b->have_v = false;
            b->recv_last.clear(); b->recv_solves = b->recv_mvps = 0; b->recv_bad = -1;
            b->mode = mode;
            return;
        }
        if (b->nsrc > 0) {
            // the memory rule of lsfc_born_set_background for what this adds, before anything is allocated
            size_t free_b = 0, total_b = 0;
            LSFC_HIP(hipMemGetInfo(&free_b, &total_b));
            const double need = reciprocal_bytes(b, b->nsrc) - (double)b->V.bytes(), vec = (double)b->N * sizeof(cplx);
            if (need > (double)free_b)
                fail(LSFC_ENOMEM, "lsfc_born_set_mode: %lld receiver fields x %lld complex (V) with the contraction's work space need %.2f GB of device memory, "
                     "%.2f GB are free -- the largest nrecv that fits is about %lld", (long long)b->nrecv, (long long)b->N, need / 1e9, (double)free_b / 1e9,
                     (long long)((double)free_b / (vec * 1.01)));
            b->mode = mode;
            bind_streams(b);
            solve_receiver_fields(b, "lsfc_born_set_mode");
            solved = true;
        }
        b->mode = mode;
    });
    if (rc == LSFC_OK && solved && b->recv_bad >= 0) {
        const int64_t keep = b->first_bad;
        b->first_bad = -1;
        const int out = not_converged(b, rc, "lsfc_born_set_mode", true);
        b->first_bad = keep;
        return out;
    }
    return rc;
}

int lsfc_born_get_mode(const lsfc_born* b, int* mode, int64_t* receiver_field_bytes) {
    return guarded([&] {
        LSFC_REQUIRE(b && mode && receiver_field_bytes, "lsfc_born_get_mode: NULL argument");
        *mode = b->mode; *receiver_field_bytes = (int64_t)b->V.bytes();
    });
}

int lsfc_born_receiver_fields(const lsfc_born* b, const double** v_dev, int64_t* nrecv) {
    return guarded([&] {
        LSFC_REQUIRE(b && v_dev && nrecv, "lsfc_born_receiver_fields: NULL argument");
        LSFC_REQUIRE(b->mode == LSFC_BORN_RECIPROCAL, "lsfc_born_receiver_fields outside reciprocal mode (lsfc_born_set_mode(LSFC_BORN_RECIPROCAL))");
        LSFC_REQUIRE(b->nsrc > 0 && b->have_v, "lsfc_born_receiver_fields before lsfc_born_set_background");
        *v_dev = (const double*)b->V.p; *nrecv = b->nrecv;
    });
}

int lsfc_born_receiver_info(const lsfc_born* b, int64_t out[4], lsfc_gmres_result* per_receiver) {
    return guarded([&] {
        LSFC_REQUIRE(b && out, "lsfc_born_receiver_info: NULL argument");
        out[0] = b->nrecv; out[1] = b->recv_solves; out[2] = b->recv_mvps; out[3] = b->recv_bad;
        if (per_receiver) for (size_t r = 0; r < b->recv_last.size(); ++r) per_receiver[r] = b->recv_last[r];
    });
}

} // extern "C"
