// Device-resident apply of the reference's SparsifyingPreconditioner (src/preconditioner.jl:27-58, 132-170):
//
//     v  <-  Msp^{-1} (As v)
//
// As is a sparse matrix (SpMV), Msp^{-1} is applied through the LU factors the caller computed on the host (UMFPACK
// `lu(Msp)` in the reference, src/preconditioner.jl:35): (Rs .* Msp)[p, q] = L U.  The factorisation itself, and the
// assembly of As / Msp, stay on the host and out of scope; what moves to the device is the part that runs once per
// Arnoldi step, so the Krylov vector no longer crosses PCIe twice per step.
//
// The two sparse triangular solves are level-scheduled (trisolve.hip).  The whole sequence SpMV -> L solve -> U solve ->
// scatter is captured once in a hipGraph on fixed internal buffers and replayed per apply.
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
#include "trisolve.hpp"
#include <algorithm>
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
    csr_row_sum<1>(rowptr[row] + lane, rowptr[row + 1], LPR, col, val, x, sx, sy);
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

__global__ void k_scatter(const cplx* __restrict__ w, const int* __restrict__ dst, cplx* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[dst[i]] = w[i];
}

// ---- host side -------------------------------------------------------------------------------------------------------

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
    ~CapturedSeq() { drop(); }
    void drop() {                      // the next replay captures again
        if (exec) (void)hipGraphExecDestroy(exec);
        if (graph) (void)hipGraphDestroy(graph);
        exec = nullptr; graph = nullptr;
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

// what an object of lsfc_precond_create holds besides As: (Rs .* Msp)[p, q] = L U from the host
struct LuRoute {
    DevBuf<int> rgather, cscatter; DevBuf<double> rscale;      // p, q (inverted for the scatter), Rs
    TriFactor *L = nullptr, *U = nullptr;
    DevBuf<cplx> z, w;                                         // L z = y0, U w = z
    ~LuRoute() { trisolve_destroy(L); trisolve_destroy(U); }
};

} // namespace lsfc

struct lsfc_precond {
    int device = 0;
    int64_t N = 0;
    hipStream_t stream = nullptr;
    lsfc::DevBuf<int64_t> a_rowptr; lsfc::DevBuf<int> a_col; lsfc::DevBuf<lsfc::cplx> a_val;     // As, CSR
    // Msp^{-1}, exactly one of the two: the host's LU factors, or the block-tridiagonal factorisation (blocktri.hip)
    lsfc::LuRoute* lu = nullptr;
    lsfc::BlockTri* bt = nullptr;
    // work vectors: [0] of the single apply; [1] of the groups of right-hand sides (block-tridiagonal objects), member-major
    // for bcap members
    lsfc::DevBuf<lsfc::cplx> vin[2], y0[2], vout[2];
    int bcap = 0;
    lsfc::DevBuf<lsfc::cplx> hstage;   // host vectors of lsfc_precond_apply and _apply_batch pass through here, grown on demand
    int launches = 0;
    int64_t bsweeps = 0, bvectors = 0, blargest = 0, bwork_bytes = 0;
    // what the applies compute (lsfc_precond_set_op): Msp^{-1} As, its transpose As^T Msp^{-T}, or its adjoint.  The
    // transposed sequence (sweeps first, then the SpMV with As^T) has graphs of its own; T and H share them, the
    // conjugations of H sit in the copies around the graph.
    int op = LSFC_OP_N;
    lsfc::BlockTriT tt{};              // the tables of the transposed apply, built by the first set_op(T | H)
    // the captured sequences, [transposed][group size]; group size 0: the single apply
    lsfc::CapturedSeq seq[2][lsfc::LSFC_MAX_BATCH + 1];
    void drop_group_graphs() {         // (those of the single apply hold addresses that stay valid)
        for (auto& s : seq) for (int R = 1; R <= lsfc::LSFC_MAX_BATCH; ++R) s[R].drop();
    }
    ~lsfc_precond() { delete lu; lsfc::blocktri_destroy(bt); }
};

namespace lsfc {

// y <- A x with A = As, or As^T for `transposed`: R = 0 one vector (an LU object gathers and scales the rows), else R members
static void launch_spmv(const lsfc_precond* pc, int R, bool transposed, const cplx* x, cplx* y, hipStream_t st) {
    const int N = (int)pc->N;
    const dim3 grid((unsigned)(((int64_t)N * 8 + 255) / 256)), block(256);
    const int64_t* rowptr = transposed ? pc->tt.rowptr : pc->a_rowptr.p;
    const int* col = transposed ? pc->tt.col : pc->a_col.p;
    const cplx* val = transposed ? pc->tt.as_val : pc->a_val.p;
    if (R == 0) {
        hipLaunchKernelGGL(k_spmv_gather<8>, grid, block, 0, st, rowptr, col, val, pc->lu ? (const int*)pc->lu->rgather.p : nullptr,
                           pc->lu ? (const double*)pc->lu->rscale.p : nullptr, x, y, N);
        return;
    }
    dispatch<1, LSFC_MAX_BATCH>(R, "preconditioner group apply", [&](auto rc) {
        hipLaunchKernelGGL(k_spmv_batch<decltype(rc)::value>, grid, block, 0, st, rowptr, col, val, x, y, N);
    });
}

// The fixed part of an apply, on internal buffers only: vout <- Msp^{-1} (As vin), or for `transposed` vout <- As^T (Msp^{-T} vin),
// the sweeps first.  R = 0: the single apply; R >= 1: a group of R members of a block-tridiagonal object (a group of one
// goes through the group kernels too, whose sums run in another order).
static void enqueue_seq(lsfc_precond* pc, int R, bool transposed, hipStream_t st) {
    const int g = R != 0, N = (int)pc->N;
    cplx *vin = pc->vin[g].p, *y0 = pc->y0[g].p, *vout = pc->vout[g].p;
    auto sweeps = [&](const cplx* w, cplx* x) {
        if (R) blocktri_enqueue_batch(pc->bt, R, w, x, st, transposed); else blocktri_enqueue(pc->bt, w, x, st, transposed);
    };
    if (transposed) { sweeps(vin, y0); launch_spmv(pc, R, true, y0, vout, st); return; }
    launch_spmv(pc, R, false, vin, y0, st);
    if (pc->bt) { sweeps(y0, vout); return; }
    const LuRoute& lu = *pc->lu;
    trisolve_enqueue(lu.L, y0, lu.z.p, st);
    trisolve_enqueue(lu.U, lu.z.p, lu.w.p, st);
    hipLaunchKernelGGL(k_scatter, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, lu.w.p, lu.cscatter.p, vout, N);
}

// v[r] (device, N complex each) <- Msp^{-1} (As v[r]), or what pc->op makes of it, stream-ordered on `st`: into the work
// vectors, the captured sequence, and back.  R = 0: the single apply of v[0], by plain copies unless the adjoint conjugates.
static void apply_seq(lsfc_precond* pc, cplx* const* v, int R, hipStream_t st) {
    const bool transposed = pc->op != LSFC_OP_N, conj = pc->op == LSFC_OP_H, plain = R == 0 && !conj;
    const int g = R != 0, cnt = R ? R : 1;
    const size_t bytes = (size_t)pc->N * sizeof(cplx);
    GroupPtrs ptrs{};
    for (int r = 0; r < cnt; ++r) ptrs.v[r] = v[r];
    const dim3 cgrid((unsigned)((pc->N + 255) / 256), (unsigned)cnt);
    if (plain) LSFC_HIP(hipMemcpyAsync(pc->vin[g].p, v[0], bytes, hipMemcpyDeviceToDevice, st));
    else if (conj) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_group_copy<true, true>), cgrid, dim3(256), 0, st, ptrs, pc->vin[g].p, pc->N);
    else hipLaunchKernelGGL(k_group_copy<true>, cgrid, dim3(256), 0, st, ptrs, pc->vin[g].p, pc->N);
    pc->seq[transposed][R].replay(st, R, [&](hipStream_t s) { enqueue_seq(pc, R, transposed, s); });
    if (plain) LSFC_HIP(hipMemcpyAsync(v[0], pc->vout[g].p, bytes, hipMemcpyDeviceToDevice, st));
    else if (conj) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_group_copy<false, true>), cgrid, dim3(256), 0, st, ptrs, pc->vout[g].p, pc->N);
    else hipLaunchKernelGGL(k_group_copy<false>, cgrid, dim3(256), 0, st, ptrs, pc->vout[g].p, pc->N);
    if (!plain) LSFC_HIP(hipGetLastError());
}

static void precond_apply_dev(lsfc_precond* pc, cplx* v, hipStream_t st) { apply_seq(pc, &v, 0, st); }

// one group of R <= LSFC_MAX_BATCH vectors of a block-tridiagonal object
static void precond_apply_group(lsfc_precond* pc, cplx* const* v, int R, hipStream_t st) {
    if (R > pc->bcap) {
        // work space on first use (and when a larger group comes): the captured graphs hold the old addresses
        LSFC_HIP(hipDeviceSynchronize());
        pc->drop_group_graphs();
        const size_t n = (size_t)R * (size_t)pc->N;
        pc->vin[1].alloc(n); pc->y0[1].alloc(n); pc->vout[1].alloc(n);
        pc->bwork_bytes = (int64_t)(3 * n * sizeof(cplx)) + blocktri_batch_reserve(pc->bt, R);
        pc->bcap = R;
    }
    apply_seq(pc, v, R, st);
    ++pc->bsweeps; pc->bvectors += R; pc->blargest = std::max<int64_t>(pc->blargest, R);
}

// pc applied to cnt >= 1 device vectors at arbitrary addresses, in place, stream-ordered on st.  A block-tridiagonal object
// takes them in groups of up to 8 through blocktri_enqueue_batch; an object of lsfc_precond_create member by member through
// the single-vector path.
static void precond_apply_batch_dev(lsfc_precond* pc, cplx* const* v, int cnt, hipStream_t st) {
    if (!pc->bt) { for (int j = 0; j < cnt; ++j) precond_apply_dev(pc, v[j], st); return; }
    for (int j0 = 0; j0 < cnt; j0 += LSFC_MAX_BATCH) precond_apply_group(pc, v + j0, std::min(LSFC_MAX_BATCH, cnt - j0), st);
}

// the preconditioner hand-off of the Krylov solvers (plan.hpp)
void plan_check_precond_op(const lsfc_plan* p, lsfc_precond_fn fn, void* precond_user, const char* who) {
    if (fn != &lsfc_precond_callback) return;
    static const char* const names[] = {"LSFC_OP_N", "LSFC_OP_T", "LSFC_OP_H"};
    const int pop = precond_user ? ((const lsfc_precond*)precond_user)->op : LSFC_OP_N;
    LSFC_REQUIRE(pop == p->op, "%s%sthe library's preconditioner object is set to %s and approximates the inverse of that form of M, the plan is set to %s: "
                 "lsfc_precond_set_op and lsfc_plan_set_op must agree", who ? who : "", who ? ": " : "", names[pop], names[p->op]);
}

Precond::Precond(lsfc_precond_fn f, void* u, bool dev, bool meet, int64_t n, const char* who)
    : fn(f), user(u), on_device(dev), own(meet && dev && f == &lsfc_precond_callback), N(n) {
    const int64_t have = own && user ? ((const lsfc_precond*)user)->N : -1;
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
        LuRoute& lu = *(pc->lu = new LuRoute());
        perm_up(lu.rgather, row_gather, "row_gather");
        perm_up(lu.cscatter, col_scatter, "col_scatter");
        if (row_scale) { lu.rscale.alloc((size_t)N); LSFC_HIP(hipMemcpy(lu.rscale.p, row_scale, (size_t)N * sizeof(double), hipMemcpyHostToDevice)); }
        lu.L = trisolve_build(N, L_rowptr, L_col, L_val, true);
        lu.U = trisolve_build(N, U_rowptr, U_col, U_val, false);
        for (DevBuf<cplx>* b : { &pc->vin[0], &pc->y0[0], &lu.z, &lu.w, &pc->vout[0] }) { b->alloc((size_t)N); LSFC_HIP(hipMemset(b->p, 0, b->bytes())); }
        pc->launches = 2 + trisolve_launches(lu.L) + trisolve_launches(lu.U);                 // SpMV, the two solves, scatter
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
        if (levels_L) *levels_L = pc->bt ? blocktri_info(pc->bt).K : trisolve_levels(pc->lu->L);
        if (levels_U) *levels_U = pc->bt ? blocktri_info(pc->bt).K : trisolve_levels(pc->lu->U);
        if (launches) *launches = pc->launches;
    });
}

int lsfc_precond_schedule(const lsfc_precond* pc, int factor, int64_t out[10]) {
    return guarded([&] {
        LSFC_REQUIRE(pc && out, "NULL argument");
        LSFC_REQUIRE(factor == 0 || factor == 1, "bad factor %d (0 = L, 1 = U)", factor);
        LSFC_REQUIRE(!pc->bt, "a block-tridiagonal preconditioner has no level schedule (see lsfc_precond_blocktri_info)");
        const int64_t* sched = trisolve_schedule(factor == 0 ? pc->lu->L : pc->lu->U);
        for (int i = 0; i < 10; ++i) out[i] = sched[i];
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
    for (DevBuf<cplx>* b : { &pc->vin[0], &pc->y0[0], &pc->vout[0] }) { b->alloc((size_t)N); LSFC_HIP(hipMemset(b->p, 0, b->bytes())); }
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
        LSFC_REQUIRE(rowptr && col && As_val && Msp_val, "NULL argument");
        LSFC_REQUIRE(memspace == LSFC_MEM_HOST || memspace == LSFC_MEM_DEVICE, "bad memspace %d", memspace);
        LSFC_REQUIRE(N >= 1 && N < ((int64_t)1 << 31), "preconditioner: N out of range");
        LSFC_REQUIRE(nblocks >= 1 && N % nblocks == 0, "block-tridiagonal preconditioner: N = %lld is not divisible by nblocks = %lld", (long long)N, (long long)nblocks);
        select_device(device, "preconditioner");
        pruned_warmup(device);
        blocktri_require_memory(N, nblocks, 0.0, "lsfc_precond_create_blocktri", bo.prec, bo.pivoting);   // from the dimensions and options alone, before any array is read
        if (memspace == LSFC_MEM_DEVICE) { *out = create_blocktri_dev(N, nblocks, rowptr, col, (const cplx*)As_val, (const cplx*)Msp_val, device, bo.prec, bo.pivoting); return; }
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
        *out = create_blocktri_dev(N, nblocks, drp.p, dcol.p, das.p, dmsp.p, device, bo.prec, bo.pivoting);
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
        LSFC_REQUIRE(plan, "NULL plan");
        LSFC_REQUIRE(!plan->dist && !plan->multi, "block-tridiagonal preconditioner: not available on a distributed or multi-device plan");
        const int64_t n = plan->dims[0], m = plan->dims[1], l = plan->ndim == 2 ? 1 : plan->dims[2];
        const int64_t N = n * m * l, K = plan->ndim == 2 ? m : l;
        int64_t nnz = 0;
        if (int rc = lsfc_sparsify_pattern(n, m, l, &nnz, nullptr, nullptr, nullptr)) fail(rc, "%s", lsfc_last_error());
        select_device(plan->device, "preconditioner");
        pruned_warmup(plan->device);
        blocktri_require_memory(N, K, (double)nnz * 40.0, "lsfc_precond_create_from_plan", bo.prec, bo.pivoting);
        DevBuf<int64_t> drp, dcol; DevBuf<cplx> das, dmsp;
        drp.alloc((size_t)N + 1); dcol.alloc((size_t)nnz); das.alloc((size_t)nnz); dmsp.alloc((size_t)nnz);
        if (int rc = lsfc_sparsify_build(plan, drp.p, dcol.p, (double*)das.p, nullptr, (double*)dmsp.p, nullptr, LSFC_MEM_DEVICE)) fail(rc, "%s", lsfc_last_error());
        *out = create_blocktri_dev(N, K, drp.p, dcol.p, das.p, dmsp.p, plan->device, bo.prec, bo.pivoting);
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
