// Restarted, left-preconditioned GMRES on the device, arithmetic of
// IterativeSolvers.jl gmres! (call sites: examples/example.jl:85,91,
// examples/example3D.jl:78): Arnoldi with modified / classical / DGKS
// Gram-Schmidt, residual estimate from the null vector of the Hessenberg matrix,
// Givens least squares at restart or convergence.  The Krylov basis stays in HBM;
// only O(restart) scalars per step cross to the host.
#include "plan.hpp"
#include "krylov_blas.hpp"
#include "team.hpp"
#include <cmath>
#include <cstdlib>
#include <complex>
#include <memory>
#include <stdexcept>
#include <vector>

namespace lsfc {

using zc = std::complex<double>;

GmresWorkspace::~GmresWorkspace() {
    if (hpin) (void)hipHostFree(hpin);
    if (vpin) (void)hipHostFree(vpin);
    for (auto& e : fetched) if (e) (void)hipEventDestroy(e);
}

// A workspace for vectors of N complex on the current device: the Krylov basis, A x, the scalars and their pinned mirror
// (vectors), the pinned host vector of a host preconditioner callback (need_vpin)
static std::unique_ptr<GmresWorkspace> new_workspace(int64_t N, int restart, bool need_vpin, bool vectors = true) {
    std::unique_ptr<GmresWorkspace> w(new GmresWorkspace());
    if (vectors) {
        w->restart = restart;
        w->V.alloc((size_t)(restart + 1) * (size_t)N);
        w->hdev.alloc((size_t)restart + 2);
        w->ydev.alloc((size_t)restart + 2);
        w->partial.alloc((size_t)blas_partial_count());
        w->ax.alloc((size_t)N);
        LSFC_HIP(hipHostMalloc((void**)&w->hpin, 2 * ((size_t)restart + 2) * sizeof(cplx)));
        for (auto& e : w->fetched) LSFC_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    if (need_vpin) LSFC_HIP(hipHostMalloc((void**)&w->vpin, (size_t)N * sizeof(cplx)));
    return w;
}

// The workspace a plan keeps across solves, grown on demand.
// vectors = false: only the pinned host vector (the root of a multi-device plan, whose Krylov basis lives in its ranks)
static GmresWorkspace* workspace(lsfc_plan* p, int restart, bool need_vpin, bool vectors = true) {
    if (!p->gmres || (vectors && p->gmres->restart < restart)) p->gmres = new_workspace(p->N, restart, false, vectors);
    if (need_vpin && !p->gmres->vpin) LSFC_HIP(hipHostMalloc((void**)&p->gmres->vpin, (size_t)p->N * sizeof(cplx)));
    return p->gmres.get();
}

// LinearAlgebra.givensAlgorithm for complex f, g: [c s; -conj(s) c] [f; g] = [r; 0], c real
static void givens(zc f, zc g, double& c, zc& s) {
    if (g == zc(0)) { c = 1.0; s = 0.0; return; }
    if (f == zc(0)) { c = 0.0; s = std::conj(g) / std::abs(g); return; }
    const double d = std::hypot(std::abs(f), std::abs(g));
    c = std::abs(f) / d;
    s = (f / std::abs(f)) * std::conj(g) / d;
}

// hessenberg.jl: least squares of the k x (k-1) Hessenberg block against beta*e1
static void solve_least_squares(const std::vector<zc>& H, int ldh, double beta, int k, std::vector<zc>& y) {
    const int width = k - 1;
    std::vector<zc> Hh((size_t)k * width), rhs((size_t)k, zc(0));
    for (int j = 0; j < width; ++j) for (int i = 0; i < k; ++i) Hh[i + (size_t)k * j] = H[i + (size_t)ldh * j];
    rhs[0] = beta;
    auto A = [&](int i, int j) -> zc& { return Hh[i + (size_t)k * j]; };
    for (int i = 0; i < width; ++i) {
        double c; zc s; givens(A(i, i), A(i + 1, i), c, s);
        A(i, i) = c * A(i, i) + s * A(i + 1, i);
        for (int j = i + 1; j < width; ++j) {
            const zc tmp = -std::conj(s) * A(i, j) + c * A(i + 1, j);
            A(i, j) = c * A(i, j) + s * A(i + 1, j);
            A(i + 1, j) = tmp;
        }
        const zc tmp = -std::conj(s) * rhs[i] + c * rhs[i + 1];
        rhs[i] = c * rhs[i] + s * rhs[i + 1];
        rhs[i + 1] = tmp;
    }
    y.assign((size_t)width, zc(0));
    for (int i = width - 1; i >= 0; --i) {
        zc acc = rhs[i];
        for (int j = i + 1; j < width; ++j) acc -= A(i, j) * y[j];
        y[i] = acc / A(i, i);
    }
}

// The solver is written once over a team of slabs (team.hpp), each holding one slab of every vector on its own device:
//   one member   ordinary plans, and one rank of a multi-PROCESS slab plan (inner products completed by ncclAllReduce)
//   P members    the ranks of a single-process multi-DEVICE plan, all driven from the calling thread
// Every vector operation is enqueued member by member; the O(restart) scalars of a step are identical on all members
// after the reduction and are read back from member 0.  What GMRES adds to a slab: its workspace, x and b.
namespace {
struct Member { lsfc_plan* p; GmresWorkspace* w; cplx* x; const cplx* b; };
struct Request;

struct Team {
    SlabTeam slabs;
    lsfc_plan* root;
    std::vector<Member> mem;            // mem[i] works on slabs.slabs[i]
    bool reduce = false;                // local inner products are partial sums
    GmresWorkspace* rootw = nullptr;    // pinned host vector of the preconditioner callback
    explicit Team(lsfc_plan* r) : slabs(r), root(r) {}

    static void dev(const Member& m) { LSFC_HIP(hipSetDevice(m.p->device)); }
    static cplx* V(const Member& m, int j) { return m.w->V.p + (size_t)j * (size_t)m.p->N; }
    // (one member: its device is made current every time, as a host callback of the caller may have left another one current)
    template <class F> void each(F&& f) { if (!slabs.multi) dev(mem[0]); slabs.each([&](const RankSlab& s) { f(mem[(size_t)s.rank]); }); }

    void apply(const Request& q);
    void allreduce(int off, int count) {
        if (!reduce) return;
        if (!root->multi) { dev(mem[0]); dist_allreduce_sum(root, mem[0].w->hdev.p + off, count); return; }
        std::vector<cplx*> ptr;
        for (auto& m : mem) ptr.push_back(m.w->hdev.p + off);
        multi_allreduce_sum(root, ptr.data(), count);
    }
    void finish_nrm(int off) {
        if (!reduce) return;
        allreduce(off, 1);
        each([&](Member& m) { blas_sqrt_dev(m.w->hdev.p + off, m.p->stream); });
    }
    // scalars of the step -> pinned host memory of member 0, slot 0 or 1: posted behind the step's kernels, awaited when
    // the host needs them (a pipelined solve posts the next step's kernels in between)
    void fetch_post(int count, int slot) {
        Member& m = mem[0];
        dev(m);
        LSFC_HIP(hipMemcpyAsync(hpin(slot), m.w->hdev.p, (size_t)count * sizeof(cplx), hipMemcpyDeviceToHost, m.p->stream));
        LSFC_HIP(hipEventRecord(m.w->fetched[slot], m.p->stream));
    }
    void fetch_wait(int slot) { dev(mem[0]); LSFC_HIP(hipEventSynchronize(mem[0].w->fetched[slot])); }
    cplx* hpin(int slot = 0) { return mem[0].w->hpin + (size_t)slot * ((size_t)mem[0].w->restart + 2); }
    void sync() { each([](Member& m) { LSFC_HIP(hipStreamSynchronize(m.p->stream)); }); }
};

// What a solve wants next: the operator on one vector of every member, then the preconditioner on Krylov column `col`.
//   init    the initial residual of a cycle, V[:,0] = Pl \ (b - A x); apply == false (initially_zero at the first start): V[:,0] = Pl \ b
//   else    expand column col: V[:,col] = Pl \ (A V[:,col-1])
struct Request {
    bool init, apply; int col;
    const cplx* in(const Member& m) const { return init ? m.x : Team::V(m, col - 1); }
    cplx* out(const Member& m) const { return init ? m.w->ax.p : Team::V(m, col); }
    bool same_kind(const Request& q) const { return init == q.init && apply == q.apply && col == q.col; }
};

void Team::apply(const Request& q) {
    std::vector<const cplx*> xi; std::vector<cplx*> yo;
    for (auto& m : mem) { xi.push_back(q.in(m)); yo.push_back(q.out(m)); }
    if (!slabs.multi) dev(mem[0]);
    slabs.apply(xi.data(), yo.data());
}

struct Resolved { lsfc_gmres_opts o; int restart; int64_t maxiter; double reltol, abstol; };
Resolved resolve(const lsfc_gmres_opts* opts_in, int64_t N) {
    Resolved r;
    if (opts_in) r.o = *opts_in;
    else { r.o.restart = 0; r.o.maxiter = 0; r.o.reltol = -1; r.o.abstol = 0; r.o.orth = LSFC_ORTH_MGS; r.o.initially_zero = 0; r.o.precond = nullptr; r.o.precond_user = nullptr; r.o.precond_on_device = 0; }
    r.restart = (int)(r.o.restart > 0 ? r.o.restart : std::min<int64_t>(20, N));
    r.maxiter = r.o.maxiter > 0 ? r.o.maxiter : N;
    r.reltol = r.o.reltol >= 0 ? r.o.reltol : DEFAULT_RELTOL;
    r.abstol = r.o.abstol > 0 ? r.o.abstol : 0.0;
    LSFC_REQUIRE(r.o.orth == LSFC_ORTH_MGS || r.o.orth == LSFC_ORTH_CGS || r.o.orth == LSFC_ORTH_DGKS, "unknown orthogonalisation %d", r.o.orth);
    LSFC_REQUIRE(r.restart >= 1, "restart must be >= 1");
    return r;
}

// One solve, cut at the operator: request() names what is to be applied and preconditioned next, applied() and post()
// enqueue the solve's own kernels behind it, consume() reads the scalars back and advances the iteration.  The driver
// does the applying and the preconditioning -- gmres_run / gmres_run_multi for one solve, gmres_run_batch for all
// running members of a batch at once.
struct Solve {
    Team& T;
    const Resolved& r; const lsfc_gmres_opts& o;
    double* resnorm; int64_t cap; lsfc_gmres_result* res;
    const int restart, ldh; const int64_t Ntot;
    bool fused, mgs_blocked, lookahead;
    std::vector<zc> H, nullvec, y;
    double beta = 0.0, current = 0.0, accumulator = 1.0, tol = 0.0;
    int k = 1;
    int posted = -1;                    // columns of this cycle whose kernels are in the stream (>= k - 1); -1: not even the initial residual
    int64_t iteration = 0, mvps;
    bool need_init = true, started = false;

    Solve(Team& team, const Resolved& rr, double* resnorm_, int64_t cap_, lsfc_gmres_result* res_, bool batch)
        : T(team), r(rr), o(rr.o), resnorm(resnorm_), cap(cap_), res(res_), restart(rr.restart), ldh(rr.restart + 1), Ntot(T.root->N),
          H((size_t)(rr.restart + 1) * rr.restart, zc(0)), nullvec((size_t)rr.restart + 1, zc(1)), mvps(rr.o.initially_zero ? 1 : 0) {
        // one device, no all-reduce between a reduction and its consumer: the fused kernels (krylov_blas.hip) sum block partials
        // inside the consuming kernel -- same summation order, bit-identical scalars, roughly half the launches
        fused = !T.reduce && T.mem.size() == 1;
        // modified Gram-Schmidt in blocks (krylov_blas.hip: k_mgs_block) where the sweep is bound by HBM traffic: vectors of >= 2^22
        // entries (LSFC_MGS_BLOCK=0 / 1 forces the strict one-vector-at-a-time sweep / the blocked one)
        const char* mb_env = getenv("LSFC_MGS_BLOCK");
        mgs_blocked = mb_env ? atoi(mb_env) != 0 : Ntot >= ((int64_t)1 << 22);
        // One step ahead: on one device nothing the host computes feeds back into the kernels of a step (the fused kernels read
        // their scalars from device memory), so the host may post step k + 1 before it has seen the scalars of step k and the
        // device never idles through the read-back, the Hessenberg update and the next launches.  The step posted past
        // convergence is surplus (its column is not used); none is posted past maxiter or past the restart length.  Worth it
        // where a step is short (small grids); off for DGKS (the host decides about the second sweep), for callbacks of
        // the caller (they would see one call more than the reference makes) -- the library's own device preconditioner
        // (lsfc_precond_callback: stream-ordered, no side effects) is fine -- and in a batch (the members post together).
        const char* lag_env = getenv("LSFC_GMRES_LOOKAHEAD");
        const bool own_precond = o.precond_on_device && o.precond == &lsfc_precond_callback;
        lookahead = fused && !batch && o.orth != LSFC_ORTH_DGKS && (!o.precond || own_precond) &&
                    (lag_env ? atoi(lag_env) != 0 : Ntot <= ((int64_t)1 << 22));
    }

    bool running() const { return need_init || !(iteration >= r.maxiter || current <= tol); }

    // steps in flight: the one the host is about to read and, with lookahead, the one after it
    bool request(Request& q) const {
        if (posted < 0) { q = { true, !(o.initially_zero && !started), 0 }; return true; }
        const int want = k + (lookahead ? 1 : 0);
        if (need_init || !(posted < want && posted < restart && iteration + (posted - (k - 1)) < r.maxiter)) return false;
        q = { false, true, posted + 1 };
        return true;
    }

    // init!: V1 = b - A x (the preconditioner comes next)
    void applied(const Request& q) {
        if (!q.init) return;
        if (q.apply) T.each([&](Member& m) { blas_sub(Team::V(m, 0), m.b, m.w->ax.p, m.p->N, m.p->stream); });
        else T.each([&](Member& m) { LSFC_HIP(hipMemcpyAsync(Team::V(m, 0), m.b, (size_t)m.p->N * sizeof(cplx), hipMemcpyDeviceToDevice, m.p->stream)); });
    }

    cplx* slot(int s2) { return T.mem[0].w->partial.p + (size_t)s2 * (size_t)blas_partial_slot(); }
    // h[j0..j0+k) = V[:, 0..k)' w  and  w -= V h   (classical Gram-Schmidt sweep over the first k columns), then ||w||
    void cgs_sweep(int k, bool scale_now, int hslot = 0, bool wait = true) {
        if (fused && k <= 64) {
            Member& m = T.mem[0];
            Team::dev(m);
            blas_multidot_partial(Team::V(m, 0), m.p->N, k, Team::V(m, k), slot(0), m.p->N, m.p->stream);
            blas_cgs_update_fused(Team::V(m, k), Team::V(m, 0), m.p->N, k, slot(0), m.w->hdev.p, slot(64), m.p->N, m.p->stream);
            if (scale_now) blas_scale_inv_fused(Team::V(m, k), slot(64), m.w->hdev.p + k, m.p->N, m.p->stream);
            else blas_finish_norm(slot(64), m.w->hdev.p + k, m.p->N, m.p->stream);
            T.fetch_post(k + 1, hslot);
            if (wait) T.fetch_wait(hslot);
            return;
        }
        T.each([&](Member& m) {
            for (int j0 = 0; j0 < k; j0 += 64) {
                const int kc = std::min(64, k - j0);
                blas_multidot(Team::V(m, j0), m.p->N, kc, Team::V(m, k), m.w->partial.p, m.w->hdev.p + j0, m.p->N, m.p->stream);
            }
        });
        T.allreduce(0, k);
        T.each([&](Member& m) {
            for (int j0 = 0; j0 < k; j0 += 64) {
                const int kc = std::min(64, k - j0);
                blas_gemv_acc(Team::V(m, k), Team::V(m, j0), m.p->N, kc, m.w->hdev.p + j0, -1.0, m.p->N, m.p->stream);
            }
            blas_nrm2(Team::V(m, k), m.w->partial.p, m.w->hdev.p + k, m.p->N, m.p->stream, T.reduce);
        });
        T.finish_nrm(k);
        if (scale_now) T.each([&](Member& m) { blas_scale_inv_dev(Team::V(m, k), m.w->hdev.p + k, m.p->N, m.p->stream); });
        T.fetch_post(k + 1, hslot);
        if (wait) T.fetch_wait(hslot);
    }

    // the solve's kernels behind the preconditioned column, and the fetch of their scalars
    void post(const Request& q) {
        posted = q.col;
        if (q.init) {
            // init!: normalise V1; beta travels to pinned slot 0
            T.each([&](Member& m) { blas_nrm2(Team::V(m, 0), m.w->partial.p, m.w->hdev.p, m.p->N, m.p->stream, T.reduce); });
            T.finish_nrm(0);
            T.each([&](Member& m) { blas_scale_inv_dev(Team::V(m, 0), m.w->hdev.p, m.p->N, m.p->stream); });
            T.fetch_post(1, 0);
            return;
        }
        // expand!: orthogonalise V[:,kk] against the columns before it; the scalars travel to pinned slot kk & 1
        const int kk = q.col, hs = kk & 1;
        if (o.orth == LSFC_ORTH_MGS && fused && mgs_blocked) {
            // blocks of MB basis vectors: one pass takes the inner products with a whole block (and of its vectors with each
            // other), the next one recovers the MGS coefficients, updates w with the block and takes the next block's products
            Member& m = T.mem[0];
            Team::dev(m);
            const int MB = blas_mgs_block_size(), S = blas_mgs_slots();
            const int nblk = (kk + MB - 1) / MB;
            blas_mgs_block(Team::V(m, kk), nullptr, 0, nullptr, nullptr, Team::V(m, 0), std::min(MB, kk), slot(0), m.p->N, m.p->N, m.p->stream);
            for (int b = 0; b < nblk; ++b) {
                const int i0 = b * MB, mp = std::min(MB, kk - i0), mn = std::max(0, std::min(MB, kk - i0 - MB));
                blas_mgs_block(Team::V(m, kk), Team::V(m, i0), mp, slot((b & 1) * S), m.w->hdev.p + i0, mn ? Team::V(m, i0 + MB) : nullptr, mn,
                               slot(((b + 1) & 1) * S), m.p->N, m.p->N, m.p->stream);
            }
            blas_scale_inv_fused(Team::V(m, kk), slot((nblk & 1) * S), m.w->hdev.p + kk, m.p->N, m.p->stream);
            T.fetch_post(kk + 1, hs);
        } else if (o.orth == LSFC_ORTH_MGS && fused) {
            Member& m = T.mem[0];
            Team::dev(m);
            blas_dot_partial(Team::V(m, 0), Team::V(m, kk), slot(0), m.p->N, m.p->stream);
            for (int i = 0; i < kk; ++i)
                blas_axpy_dot_fused(Team::V(m, kk), Team::V(m, i), slot(i & 1), m.w->hdev.p + i, (i + 1 < kk) ? Team::V(m, i + 1) : nullptr,
                                    slot((i + 1) & 1), m.p->N, m.p->stream);
            blas_scale_inv_fused(Team::V(m, kk), slot(kk & 1), m.w->hdev.p + kk, m.p->N, m.p->stream);
            T.fetch_post(kk + 1, hs);
        } else if (o.orth == LSFC_ORTH_MGS) {
            // h_i = <V_i, w>; w -= h_i V_i, each sweep fused with the next inner product (norm after the last)
            T.each([&](Member& m) { blas_dot(Team::V(m, 0), Team::V(m, kk), m.w->partial.p, m.w->hdev.p, m.p->N, m.p->stream); });
            T.allreduce(0, 1);
            for (int i = 0; i < kk; ++i) {
                T.each([&](Member& m) {
                    blas_axpy_dot(Team::V(m, kk), Team::V(m, i), m.w->hdev.p + i, (i + 1 < kk) ? Team::V(m, i + 1) : nullptr, m.w->partial.p,
                                  m.w->hdev.p + i + 1, m.p->N, m.p->stream, T.reduce);
                });
                if (i + 1 < kk) T.allreduce(i + 1, 1); else T.finish_nrm(i + 1);
            }
            T.each([&](Member& m) { blas_scale_inv_dev(Team::V(m, kk), m.w->hdev.p + kk, m.p->N, m.p->stream); });
            T.fetch_post(kk + 1, hs);
        } else {
            cgs_sweep(kk, o.orth == LSFC_ORTH_CGS, hs, false);
        }
    }

    // the oldest fetch in flight: beta of a (re)start, or step k
    void consume() {
        if (need_init) {
            T.fetch_wait(0);
            beta = T.hpin()[0].x;
            accumulator = 1.0;
            nullvec[0] = 1.0;
            if (started) ++mvps;
            else { current = beta; tol = std::max(r.reltol * current, r.abstol); started = true; }
            need_init = false;
            return;
        }
        ++mvps;
        double nrm;
        cplx* hp = T.hpin(k & 1);
        T.fetch_wait(k & 1);
        nrm = hp[k].x;
        if (o.orth == LSFC_ORTH_DGKS) {
            // IterativeSolvers orthogonalize.jl: `while nrm < projection_size / sqrt(2)`, projection_size being
            // the norm of the latest correction; the corrections accumulate into the Hessenberg column
            double proj = 0.0;
            for (int i = 0; i < k; ++i) proj += hp[i].x * hp[i].x + hp[i].y * hp[i].y;
            proj = std::sqrt(proj);
            std::vector<cplx> hsum(hp, hp + k);
            bool again = false;
            for (int pass = 0; nrm < proj / std::sqrt(2.0) && pass < 8; ++pass) {     // (8: guard against a stagnating loop)
                again = true;
                cgs_sweep(k, false, k & 1, true);
                proj = 0.0;
                for (int i = 0; i < k; ++i) {
                    proj += hp[i].x * hp[i].x + hp[i].y * hp[i].y;
                    hsum[(size_t)i].x += hp[i].x; hsum[(size_t)i].y += hp[i].y;
                }
                proj = std::sqrt(proj);
                nrm = hp[k].x;
            }
            if (again) for (int i = 0; i < k; ++i) hp[i] = hsum[(size_t)i];
            T.each([&](Member& m) { blas_scale_inv_dev(Team::V(m, k), m.w->hdev.p + k, m.p->N, m.p->stream); });
        }
        for (int i = 0; i < k; ++i) H[i + (size_t)ldh * (k - 1)] = zc(hp[i].x, hp[i].y);
        H[k + (size_t)ldh * (k - 1)] = nrm;

        // update_residual!: nullvec[k+1] = -conj(dot(nullvec[1:k], H[1:k,k]) / H[k+1,k])
        zc acc(0);
        for (int i = 0; i < k; ++i) acc += std::conj(nullvec[i]) * H[i + (size_t)ldh * (k - 1)];
        nullvec[k] = -std::conj(acc / nrm);
        // an exhausted Krylov space (H[k+1,k] == 0, or an entry that overflows) holds the exact solution: converged, as
        // numpy's abs(inf + nan im)^2 == inf has it, where std::norm gives NaN (GMRES); the least squares
        // below uses columns 1..k only, so the unnormalisable v_{k+1} is never read
        if (nrm == 0.0 || !std::isfinite(nullvec[k].real()) || !std::isfinite(nullvec[k].imag())) current = 0.0;
        else {
            accumulator += std::norm(nullvec[k]);
            current = beta / std::sqrt(accumulator);
        }
        ++k;

        if (k == restart + 1 || current <= tol) {
            solve_least_squares(H, ldh, beta, k, y);
            T.sync();                                       // (members other than 0 may still read their pinned scalars)
            T.each([&](Member& m) {
                for (int i = 0; i < k - 1; ++i) m.w->hpin[i] = make_double2(y[i].real(), y[i].imag());
                LSFC_HIP(hipMemcpyAsync(m.w->ydev.p, m.w->hpin, (size_t)(k - 1) * sizeof(cplx), hipMemcpyHostToDevice, m.p->stream));
                for (int j0 = 0; j0 < k - 1; j0 += 64) {
                    const int kc = std::min(64, k - 1 - j0);
                    blas_gemv_acc(m.x, Team::V(m, j0), m.p->N, kc, m.w->ydev.p + j0, +1.0, m.p->N, m.p->stream);      // x += V y
                }
            });
            T.sync();
            // a cycle that ended above the tolerance starts the next one, whatever maxiter says: the reference's order
            need_init = !(current <= tol);
            k = 1; posted = need_init ? -1 : 0;
        }
        if (resnorm && iteration < cap) resnorm[iteration] = current;
        ++iteration;
    }

    void finish() { res->iters = iteration; res->mvps = mvps; res->converged = current <= tol ? 1 : 0; res->final_resnorm = current; }
};

// the preconditioner on Krylov column `col` of one solve
void precondition(Team& T, const Precond& pc, int col) {
    if (!pc.fn) return;
    if (pc.on_device) LSFC_REQUIRE(T.mem.size() == 1, "a device-resident preconditioner callback needs a single-device plan");
    if (T.mem.size() == 1) {
        Member& m = T.mem[0];
        Team::dev(m);
        cplx* const v = Team::V(m, col);
        pc.apply(&v, 1, T.rootw->vpin, m.p->stream);
        return;
    }
    T.slabs.host_precond(pc, T.rootw->vpin, [&](const RankSlab& s) { return Team::V(T.mem[(size_t)s.rank], col); });
}

// one solve over a team
void solve(Team& T, const Resolved& r, double* resnorm, int64_t cap, lsfc_gmres_result* res) {
    plan_check_precond_op(T.root, r.o.precond, r.o.precond_user, nullptr);
    Solve S(T, r, resnorm, cap, res, false);
    const Precond pc(r.o.precond, r.o.precond_user, r.o.precond_on_device != 0, false, T.root->N, nullptr);   // (a single solve meets nobody)
    while (S.running()) {
        for (Request q; S.request(q);) {
            if (q.apply) T.apply(q);
            S.applied(q);
            precondition(T, pc, q.col);
            S.post(q);
        }
        S.consume();
    }
    T.sync();
    S.finish();
}
} // namespace

void gmres_run(lsfc_plan* p, cplx* x, const cplx* b, const lsfc_gmres_opts* opts_in, double* resnorm, int64_t cap, lsfc_gmres_result* res) {
    const Resolved r = resolve(opts_in, p->N);
    Team T(p);
    GmresWorkspace* w = workspace(p, r.restart, r.o.precond != nullptr && !r.o.precond_on_device);
    T.mem.push_back({p, w, x, b});
    T.rootw = w;
    // slab-distributed plan (one process per GPU): every inner product / squared norm is completed by an all-reduce over the ranks
    T.reduce = p->dist && !p->dist->sim && !p->dist->member && (p->dist->nranks > 1 || p->dist->force_comm);
    solve(T, r, resnorm, cap, res);
}

// Lock step, on the calling thread.  All running members are always in the same phase -- they start together, the restart
// comes at the same k for every member and costs each of them one operator application, DGKS applies none, and a member
// only ever leaves -- so a round is: one request per member (all of one kind), the operator on all of them in groups that
// share a pass of the pipeline, the preconditioner (Precond::apply), every member's kernels, and only then the scalars of each.
void gmres_run_batch(lsfc_plan* p, cplx* x, const cplx* b, int nrhs, const lsfc_gmres_opts* opts_in, double* resnorm, int64_t cap,
                     lsfc_gmres_result* res) {
    const Resolved r = resolve(opts_in, p->N);
    plan_check_precond_op(p, r.o.precond, r.o.precond_user, nullptr);
    const Precond pc(r.o.precond, r.o.precond_user, r.o.precond_on_device != 0, true, p->N, nullptr);
    // one workspace (Krylov basis, scalars, pinned buffers) per right-hand side: nrhs * (restart + 2) vectors of N complex.
    // Checked against the free device memory up front (a failed hipMalloc half way through leaves a half-built batch), and
    // released again when the call returns -- the single-solve workspace of the plan is the one that is kept across calls.
    {
        size_t free_b = 0, total_b = 0;
        LSFC_HIP(hipMemGetInfo(&free_b, &total_b));
        const double need = (double)nrhs * ((double)r.restart + 2.0) * (double)p->N * sizeof(cplx);
        if (need > (double)free_b)
            fail(LSFC_ENOMEM, "lsfc_gmres_batch: %d right-hand sides x (restart %d + 2) vectors of %lld complex need %.1f GB of device memory, %.1f GB are free "
                 "-- solve fewer right-hand sides per call or lower the restart length", nrhs, r.restart, (long long)p->N, need / 1e9, (double)free_b / 1e9);
    }
    std::vector<std::unique_ptr<GmresWorkspace>> ws;
    for (int j = 0; j < nrhs; ++j) ws.push_back(new_workspace(p->N, r.restart, pc.fn && !pc.on_device && j == 0));      // (one pinned vector serves every member's callback)
    LSFC_HIP(hipStreamSynchronize(p->stream));
    std::vector<Team> teams((size_t)nrhs, Team(p));
    std::vector<Solve> S;
    S.reserve((size_t)nrhs);
    std::vector<Solve*> act;
    for (int j = 0; j < nrhs; ++j) {
        Team& T = teams[(size_t)j];
        T.mem.push_back({p, ws[(size_t)j].get(), x + (int64_t)j * p->N, b + (int64_t)j * p->N});
        S.emplace_back(T, r, resnorm ? resnorm + (int64_t)j * cap : nullptr, cap, res + j, true);
        act.push_back(&S.back());
    }
    try {
        std::vector<Request> q;
        std::vector<const cplx*> in; std::vector<cplx*> out, col;
        while (!act.empty()) {
            q.resize(act.size()); in.clear(); out.clear(); col.clear();
            for (size_t a = 0; a < act.size(); ++a) {
                const Member& m = act[a]->T.mem[0];
                if (!act[a]->request(q[a]) || !q[a].same_kind(q[0])) throw std::logic_error("lsfc_gmres_batch: the members of a round are not in the same phase");
                in.push_back(q[a].in(m)); out.push_back(q[a].out(m)); col.push_back(Team::V(m, q[a].col));
            }
            if (q[0].apply) plan_apply_batch_dev(p, in.data(), out.data(), in.size());
            for (size_t a = 0; a < act.size(); ++a) act[a]->applied(q[a]);
            pc.apply(col.data(), col.size(), ws[0]->vpin, p->stream);
            for (size_t a = 0; a < act.size(); ++a) act[a]->post(q[a]);
            size_t kept = 0;
            for (Solve* s : act) { s->consume(); if (s->running()) act[kept++] = s; }
            act.resize(kept);
        }
    } catch (...) {
        (void)hipStreamSynchronize(p->stream);              // the workspaces are about to go
        throw;
    }
    LSFC_HIP(hipStreamSynchronize(p->stream));
    for (auto& s : S) s.finish();
}

void gmres_run_multi(lsfc_plan* root, cplx* x_host, const cplx* b_host, const lsfc_gmres_opts* opts_in, double* resnorm, int64_t cap,
                     lsfc_gmres_result* res) {
    LSFC_REQUIRE(root->multi, "not a multi-device plan");
    const Resolved r = resolve(opts_in, root->N);
    LSFC_REQUIRE(!(r.o.precond && r.o.precond_on_device), "a multi-device plan takes a host preconditioner callback");
    Team T(root);
    T.rootw = workspace(root, r.restart, r.o.precond != nullptr, false);
    T.reduce = root->multi->P > 1;
    T.slabs.scatter(x_host, b_host);
    T.slabs.each([&](const RankSlab& s) { T.mem.push_back({s.p, workspace(s.p, r.restart, false), s.p->xs.p, s.p->ys.p}); });
    solve(T, r, resnorm, cap, res);
    T.slabs.gather(x_host);
    T.sync();
    LSFC_HIP(hipSetDevice(root->device));
}

} // namespace lsfc

using namespace lsfc;

extern "C" int lsfc_gmres(lsfc_plan* plan, double* x, const double* b, const lsfc_gmres_opts* opts, double* resnorm, int64_t resnorm_cap,
                          lsfc_gmres_result* result, int memspace) {
    int conv_code = LSFC_OK;
    int rc = guarded([&] {
        LSFC_REQUIRE(plan && x && b, "NULL argument");
        LSFC_HIP(hipSetDevice(plan->device));
        lsfc_gmres_result local; lsfc_gmres_result* res = result ? result : &local;
        if (plan->multi) {
            LSFC_REQUIRE(memspace == LSFC_MEM_HOST, "a multi-device plan takes host vectors");
            gmres_run_multi(plan, (cplx*)x, (const cplx*)b, opts, resnorm, resnorm_cap, res);
        } else if (memspace == LSFC_MEM_DEVICE) {
            gmres_run(plan, (cplx*)x, (const cplx*)b, opts, resnorm, resnorm_cap, res);
        } else {
            LSFC_REQUIRE(memspace == LSFC_MEM_HOST, "unknown memspace %d", memspace);
            plan_ensure_staging(plan, plan->N);
            LSFC_HIP(hipMemcpy(plan->xs.p, x, plan->N * sizeof(cplx), hipMemcpyHostToDevice));
            LSFC_HIP(hipMemcpy(plan->ys.p, b, plan->N * sizeof(cplx), hipMemcpyHostToDevice));
            gmres_run(plan, plan->xs.p, plan->ys.p, opts, resnorm, resnorm_cap, res);
            LSFC_HIP(hipMemcpy(x, plan->xs.p, plan->N * sizeof(cplx), hipMemcpyDeviceToHost));
        }
        if (!res->converged) conv_code = LSFC_ENOTCONV;
    });
    if (rc == LSFC_OK && conv_code != LSFC_OK) { set_last_error("gmres: maxiter reached without convergence"); return conv_code; }
    return rc;
}

extern "C" int lsfc_gmres_batch(lsfc_plan* plan, double* x, const double* b, int64_t nrhs, const lsfc_gmres_opts* opts, double* resnorm,
                                int64_t resnorm_cap, lsfc_gmres_result* results, int memspace) {
    return guarded([&] {
        LSFC_REQUIRE(plan && x && b && results, "NULL argument");
        LSFC_REQUIRE(nrhs >= 1 && nrhs <= KRYLOV_NRHS_MAX, "nrhs must be in 1..%d", KRYLOV_NRHS_MAX);
        LSFC_REQUIRE(!plan->multi && !plan->dist, "batched GMRES runs on a single-device plan");
        LSFC_HIP(hipSetDevice(plan->device));
        if (memspace == LSFC_MEM_DEVICE) {
            gmres_run_batch(plan, (cplx*)x, (const cplx*)b, (int)nrhs, opts, resnorm, resnorm_cap, results);
        } else {
            LSFC_REQUIRE(memspace == LSFC_MEM_HOST, "unknown memspace %d", memspace);
            const size_t bytes = (size_t)nrhs * plan->N * sizeof(cplx);
            DevBuf<cplx> xd, bd; xd.alloc((size_t)nrhs * plan->N); bd.alloc((size_t)nrhs * plan->N);
            LSFC_HIP(hipMemcpy(xd.p, x, bytes, hipMemcpyHostToDevice));
            LSFC_HIP(hipMemcpy(bd.p, b, bytes, hipMemcpyHostToDevice));
            gmres_run_batch(plan, xd.p, bd.p, (int)nrhs, opts, resnorm, resnorm_cap, results);
            LSFC_HIP(hipMemcpy(x, xd.p, bytes, hipMemcpyDeviceToHost));
        }
    });
}
