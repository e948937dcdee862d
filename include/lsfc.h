/*
 * lsfc.h -- C ABI of the MI355X-native Lippmann-Schwinger fast-convolution
 * operator (y = x + omega^2 * G * (nu .* x)) and the GMRES loop that drives it.
 *
 * This is the drop-in boundary for ONE hot path of
 * tanderson92/Fast_solver_Lippmann_Schwinger: the FastM / FastM3D operator
 * apply and the IterativeSolvers.gmres! loop.  Every entry point names the
 * reference interface it replaces (paths relative to the reference root).
 * INTEGRATION.md shows the Julia `ccall` stubs a maintainer would add.
 *
 * Conventions (identical to the reference):
 *   - all grid functions are flat vectors in column-major order, x fastest
 *     (examples/example.jl:39-40, examples/example3D.jl:33-39);
 *   - complex numbers are interleaved (re, im) doubles == Julia Complex{Float64};
 *   - every function returns 0 on success, a negative LSFC_E* code on failure;
 *     the message is available through lsfc_last_error(); no C++ exception
 *     crosses this boundary;
 *   - a plan is not thread-safe; calls are synchronous on return for host
 *     buffers and stream-ordered (plan stream) for device buffers.
 *
 * There is no CPU fallback behind this ABI: every compute entry point runs
 * HIP kernels on a gfx950 device and fails with LSFC_ENODEV when none is present.
 */
#ifndef LSFC_H
#define LSFC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lsfc_plan lsfc_plan;

/* error codes */
#define LSFC_OK        0
#define LSFC_EINVAL   -1   /* bad argument (the reference would throw DimensionMismatch / UndefVarError) */
#define LSFC_ENODEV   -2   /* no HIP device */
#define LSFC_ENOMEM   -3
#define LSFC_EHIP     -4   /* HIP / rocFFT / RCCL runtime failure */
#define LSFC_ENOTCONV -5   /* GMRES hit maxiter without converging (x still updated, like gmres!); BiCGStab(l): cap or breakdown */

/* quadRule (src/FastConvolution.jl:20, src/FastConvolution3D.jl:21) */
#define LSFC_QUAD_TRAPEZOIDAL     0   /* "trapezoidal"    */
#define LSFC_QUAD_GREENGARD_VICO  1   /* "Greengard_Vico" */

/* where the caller's vectors live */
#define LSFC_MEM_HOST    0
#define LSFC_MEM_DEVICE  1

/* plan flags */
#define LSFC_FLAG_DEFAULT        0u
#define LSFC_FLAG_LITERAL_PAD    1u   /* keep the reference's literal (ne,me,le) padded grid + shifts
                                         (rocFFT path; for parity tests of the padding identity) */
#define LSFC_FLAG_FORCE_ROCFFT   2u   /* reduced grid, but monolithic rocFFT transforms instead of
                                         the hand-written pruned pipeline */
#define LSFC_FLAG_PATCH_SINGULAR 4u   /* builders only: replace the removable 0/0 of the symbol at
                                         |s| == k by its analytic limit (reference yields Inf/NaN) */

/* orthogonalisation (IterativeSolvers.jl orth_meth) */
#define LSFC_ORTH_MGS   0   /* ModifiedGramSchmidt() -- gmres! default */
#define LSFC_ORTH_CGS   1   /* ClassicalGramSchmidt() */
#define LSFC_ORTH_DGKS  2   /* DGKS() */

/* ---- plan construction -------------------------------------------------- */

/* Replaces the constructor FastM(GFFT,nu,ne,me,n,m,k; quadRule)
 * (src/FastConvolution.jl:11-27).  gfft: ne*me interleaved complex, column-major,
 * in the reference's layout: centred (fftshift) order for Greengard_Vico, plain
 * FFT order for trapezoidal.  nu: n*m doubles.  Both are copied (host pointers). */
int lsfc_plan_create_2d(lsfc_plan** out, int64_t n, int64_t m, int64_t ne, int64_t me,
                        const double* nu, const double* gfft, double omega,
                        int quad_rule, unsigned flags, int device);

/* Replaces FastM3D(GFFT,nu,ne,me,le,n,m,l,k; quadRule) (src/FastConvolution3D.jl:7-26). */
int lsfc_plan_create_3d(lsfc_plan** out, int64_t n, int64_t m, int64_t l,
                        int64_t ne, int64_t me, int64_t le,
                        const double* nu, const double* gfft, double omega,
                        int quad_rule, unsigned flags, int device);

/* Replaces buildFastConvolution(x,y,h,k,nu; quadRule="Greengard_Vico")
 * (src/FastConvolution.jl:170-236 + Gtruncated2D, src/Functions.jl:40-42).
 * box = |x[end]-x[1]| + h; nu already evaluated on the grid (n*m doubles).
 * The symbol is generated on the device. */
int lsfc_plan_create_gv2d(lsfc_plan** out, int64_t n, int64_t m, double box, double omega,
                          const double* nu, unsigned flags, int device);

/* Replaces buildFastConvolution(x,y,h,k,nu; quadRule="trapezoidal")
 * (src/FastConvolution.jl:172-183, buildGConv :425-469).  Odd n,m only, as the
 * reference.  x0,y0 = x[1],y[1]; d0 = D[round(Int,k*h)] (re,im). */
int lsfc_plan_create_trap2d(lsfc_plan** out, int64_t n, int64_t m, double x0, double y0, double h,
                            double omega, double d0_re, double d0_im,
                            const double* nu, unsigned flags, int device);

/* Replaces buildFastConvolution3D(x,y,z,X,Y,Z,h,k,nu) (src/FastConvolution3D.jl:68-101
 * + Gtruncated3D, src/Functions.jl:49-51).  The (4n)^3 symbol cube of the
 * reference (137 GB at n=512) is never materialised: the symbol is evaluated
 * slab-wise on the device and reduced to the equivalent (2n)^3 grid.
 * box = |x[end] - x[1]| + h: as in the reference (:72-81), the truncation radius and the frequency lattice of ALL three
 * axes derive from the x extent, so the symbol is the physical truncated kernel only when n == m == l (the reference's
 * own use); for other shapes the reference's arithmetic is reproduced as it is. */
int lsfc_plan_create_gv3d(lsfc_plan** out, int64_t n, int64_t m, int64_t l, double box, double omega,
                          const double* nu, unsigned flags, int device);

int lsfc_plan_destroy(lsfc_plan* plan);

/* ---- operator traits (src/FastConvolution.jl:31-41) ----------------------- */

/* size(M, dim) == length(nu) */
int64_t lsfc_plan_size(const lsfc_plan* plan);
/* dims[0..2] = n,m,l (l = 1 in 2D); pads[0..2] = working padded grid actually used */
int lsfc_plan_dims(const lsfc_plan* plan, int64_t dims[3], int64_t pads[3]);
/* name of the transform pipeline in use: "pruned-hip", "rocfft-reduced", "rocfft-literal" */
const char* lsfc_plan_pipeline(const lsfc_plan* plan);
/* replace the contrast (nu is a mutable field of the reference struct).  N doubles: the plan's nu is REAL from here on (after
 * lsfc_plan_set_nu_complex this frees the imaginary plane, and every result is bit for bit that of a plan that never saw a
 * complex nu). */
int lsfc_plan_set_nu(lsfc_plan* plan, const double* nu, int memspace);
/* Complex nu: an absorbing (lossy) medium.  This goes beyond the reference, whose nu is an Array{Float64,1}.
 * nu: N (re, im) pairs, interleaved like every complex vector of this ABI.  The plan's nu is complex from here on.
 * The creators take a real nu: a complex plan is a created plan plus one call of this entry.  The plan keeps Re nu and Im nu
 * as two planes of N doubles (the real path keeps its 8 B per point and its instructions); every entry that reads the plan's
 * nu honours both: lsfc_apply, lsfc_apply_batch modes 0 and 2, lsfc_convolve with apply_nu, lsfc_time_apply,
 * lsfc_profile_apply (whose byte model counts 16 B per point of nu), host and device vectors alike, lsfc_sparsify_build
 * (Msp = As + omega^2 AG diag(nu), a complex multiply-add), lsfc_precond_create_from_plan* and the four Krylov entry points.
 * M^T and M^H with a complex nu: see lsfc_plan_set_op below.
 * After an error of this entry the plan has the nu it had before the call.
 * LSFC_EINVAL: NULL argument (before any device call); a distributed, simulated-rank or multi-device plan ("complex nu is not
 * available on ..."; such a plan keeps working with its real nu). */
int lsfc_plan_set_nu_complex(lsfc_plan* plan, const double* nu, int memspace);
/* *is_complex = 1 after lsfc_plan_set_nu_complex, 0 after a creator or lsfc_plan_set_nu */
int lsfc_plan_nu_is_complex(const lsfc_plan* plan, int* is_complex);
/* copy the working symbol out (debug / tests): count complex entries written */
int lsfc_plan_get_symbol(const lsfc_plan* plan, double* out, int64_t capacity_complex, int64_t* count);
/* The order in which the hand-written passes keep a line of L points (debug / tests; with it and the last line of
 * lsfc_plan_describe_passes the working symbol decodes to natural order): freq_of_slot[s] = frequency index, 0 .. L-1, held at
 * storage slot s, for s < L.  Pure host arithmetic, no device needed.  LSFC_EINVAL: NULL, or a length that the pipeline does not
 * have (anything but 2^k, 3*2^k, 5*2^k of lsfc_padded_length). */
int lsfc_storage_order(int64_t L, int64_t* freq_of_slot);

/* ---- the apply ------------------------------------------------------------ */

/* y = x + omega^2 * FFTconvolution(nu .* x): replaces `*`, `mul!`, `fastconvolution`
 * (src/FastConvolution.jl:43-107) and `*(M::FastM3D,b)` (src/FastConvolution3D.jl:31-37).
 * x, y: N interleaved complex; y may alias x. */
int lsfc_apply(lsfc_plan* plan, const double* x, double* y, int memspace);

/* y = crop(ifft(GFFT .* fft(pad(apply_nu ? nu.*x : x)))): replaces FFTconvolution
 * (src/FastConvolution.jl:110-154, src/FastConvolution3D.jl:39-63).  The reference
 * multiplies by nu in the 2D trapezoidal branch only; the host wrapper passes
 * apply_nu accordingly. */
int lsfc_convolve(lsfc_plan* plan, const double* x, double* y, int apply_nu, int memspace);

/* nrhs independent applies, vectors stored back to back (x + j*N).  Serves the multi-source callers (sampleG3D applies
 * the operator to up to 27 unit vectors at a time, src/FastConvolution3D.jl:146-159) and several incident fields
 * (tests/plasma_example.jl:160-176).  Groups of up to 8 right-hand sides go through ONE pass of the pipeline: the x and
 * y passes run all of them per launch and the fused pass loads each tile of the Green's symbol once per group, so the
 * symbol's share of the HBM traffic (8 of the 35 complex per point in the byte model) is paid once per group instead of
 * once per vector, and small grids amortise their launch latency. */
int lsfc_apply_batch(lsfc_plan* plan, const double* x, double* y, int64_t nrhs, int mode /*0 apply,1 convolve,2 convolve+nu*/, int memspace);

/* Rows of the discrete Green's matrix for the delta sources at grid indices sources[0..nsrc): out + s*N receives
 * FFTconvolution(M, e_{sources[s]}).  Replaces sampleGConv / sampleG3D(..., fastconv) (src/FastConvolution.jl:278-306,
 * src/FastConvolution3D.jl:136-160), which run one full FFT convolution per source (O(10^3) of them in the
 * preconditioner set-up).  Here the spatial kernel is obtained ONCE (one convolution of a unit source at index 0)
 * and every row is a gather K[|i - j|] -- the kernel is even in every axis -- so the cost per source is one
 * N-vector write.  (2D trapezoidal plans: as in the reference's FFTconvolution, nu is NOT applied to a delta row
 * by this entry; use lsfc_apply_batch for that quirk.)
 * The gather is a row of G only for a kernel that is even along every axis on its own, K(-dx, dy, dz) = K(dx, dy, dz) and so
 * on.  The kernels of lsfc_plan_create_gv2d / gv3d are, and that of lsfc_plan_create_trap2d on a grid centred at the origin
 * (x0 = -(n-1) h / 2, y0 = -(m-1) h / 2); they pay nothing.  Any other plan (lsfc_plan_create_2d / 3d take any symbol) is
 * measured at the first call of this entry or of lsfc_sparsify_build, once per plan: one convolution of a unit source at each
 * other corner of the grid (3 in 2D, 7 in 3D), compared with the response at index 0 mirrored, as max |difference| over the
 * largest entry of the kernel.  Above 1e-10: LSFC_EINVAL, the message names the axis and the deviation, nothing is written.
 * This is stronger than the symmetry of G that lsfc_plan_set_op asks for: G(-k) = G(k) over all axes jointly makes G
 * symmetric and passes there, and is refused here. */
int lsfc_sample_sources(lsfc_plan* plan, const int64_t* sources, int64_t nsrc, double* out, int memspace);

/* ---- the transposed and the adjoint operator ------------------------------ */

/* omega is real and the Green's matrix G of every builder is complex symmetric, so
 *     M^T = I + omega^2 diag(nu) G        and        M^H y = conj(M^T conj(y)) = y + omega^2 conj(nu) .* conj(G conj(y)).
 * nu may be complex (lsfc_plan_set_nu_complex).  The rule is: THE CONJUGATION IS OUTERMOST.  M^T multiplies by nu itself,
 * M^H by conj(nu); whatever describes G and the nu multiply literally (lsfc_convolve with apply_nu, lsfc_apply_batch mode 2,
 * the trapezoidal FFTconvolution quirk) multiplies by nu itself under every op.
 * In the pipeline only the nu multiply moves, from the loads of the first x pass to the stores of the last one; M^H adds
 * two conjugations there.  The y passes, the fused pass and the HBM traffic per point are those of M.
 *
 * The op is plan state (default LSFC_OP_N).  It is READ by everything that means "the operator": lsfc_apply,
 * lsfc_apply_batch mode 0, lsfc_time_apply, lsfc_profile_apply and every operator application inside lsfc_gmres,
 * lsfc_gmres_batch, lsfc_bicgstabl and lsfc_bicgstabl_batch.  It is NOT read by lsfc_convolve, lsfc_apply_batch modes 1
 * and 2, lsfc_sample_sources, lsfc_sparsify_build and lsfc_precond_create_from_plan: those keep describing G and M.
 *
 * I + omega^2 diag(nu) G is the transpose only when G is symmetric, and lsfc_plan_create_2d/3d take any symbol.  So the first
 * lsfc_plan_set_op(T | H) or lsfc_plan_symmetry_defect of a plan measures, through the plan's own convolution,
 *     defect = |sum y.*(G x) - sum x.*(G y)| / (||G x|| ||y||)
 * for two fixed unit-modulus probe vectors generated on the device from the grid index (the same in every run), and keeps
 * the figure.  defect > 1e-10: lsfc_plan_set_op returns LSFC_EINVAL, the message names the defect, and the op stays N
 * (symmetric operators measure ~1e-16, non-symmetric ones ~1e-2 and more).
 *
 * LSFC_EINVAL, before any device call: NULL plan; op outside 0..2; a distributed, simulated-rank or multi-device plan.
 * A solve whose preconditioner is the library's own object (precond == lsfc_precond_callback) is accepted if and only if
 * the object's op (lsfc_precond_set_op below, default N) equals the plan's; otherwise it returns LSFC_EINVAL and the
 * message names both ops.  Caller callbacks pass through unchanged.
 *
 * The transposed and the adjoint preconditioner As^T Msp^-T exist for block-tridiagonal objects (lsfc_precond_set_op).
 * Out of scope: the transposed apply of an object of lsfc_precond_create (host LU factors); right
 * preconditioning; distributed and multi-device plans; non-symmetric kernels (they would need the reflected symbol). */
#define LSFC_OP_N 0   /* M           (default)                         */
#define LSFC_OP_T 1   /* transpose   I + w^2 diag(nu) G                */
#define LSFC_OP_H 2   /* adjoint     conj(T conj(.))                   */
int lsfc_plan_set_op(lsfc_plan* plan, int op);
int lsfc_plan_get_op(const lsfc_plan* plan, int* op);
int lsfc_plan_symmetry_defect(lsfc_plan* plan, double* defect);

/* ---- GMRES ---------------------------------------------------------------- */

/* In-place left preconditioner, mirrors the two-argument ldiv!(Pl, v)
 * (src/preconditioner.jl:147-170): v holds N interleaved complex on the HOST and
 * is overwritten with Pl \ v.  Called synchronously on the calling thread once
 * per Arnoldi step (and once per (re)start).  Return non-zero to abort. */
typedef int (*lsfc_precond_fn)(void* user, double* v, int64_t n);

typedef struct lsfc_gmres_opts {
    int     restart;       /* <=0: min(20, N)                       */
    int64_t maxiter;       /* <=0: N                                 */
    double  reltol;        /* <0: sqrt(eps)                          */
    double  abstol;        /* default 0                              */
    int     orth;          /* LSFC_ORTH_*                            */
    int     initially_zero;/* skip the initial A*x0 (x0 == 0)        */
    lsfc_precond_fn precond; void* precond_user;  /* NULL: Identity() */
    int     precond_on_device; /* 0 (default): v is a HOST pointer (copied over PCIe around the call, like the
                                  reference's host-side ldiv!).  1: v is the DEVICE pointer of the Krylov vector
                                  itself; the callback must enqueue its work on the plan's stream (or synchronise)
                                  -- the hook for a device-resident preconditioner, no PCIe traffic. */
} lsfc_gmres_opts;

typedef struct lsfc_gmres_result {
    int64_t iters;         /* inner iterations performed (history.iters)            */
    int64_t mvps;          /* operator applications (history.mvps)                  */
    int     converged;     /* history.isconverged                                   */
    double  final_resnorm; /* last implicit (preconditioned) residual norm          */
} lsfc_gmres_result;

/* Replaces IterativeSolvers.gmres!(x, fastconv, b; Pl, restart, reltol, abstol,
 * maxiter, log=true) as called at examples/example.jl:85,91 and
 * examples/example3D.jl:78.  x (in/out) and b: N complex.  resnorm (may be NULL)
 * receives up to resnorm_cap entries of history[:resnorm]. */
int lsfc_gmres(lsfc_plan* plan, double* x, const double* b, const lsfc_gmres_opts* opts,
               double* resnorm, int64_t resnorm_cap, lsfc_gmres_result* result, int memspace);

/* nrhs independent solves of the same operator in lock step (x, b: nrhs vectors back to back; resnorm: nrhs rows of
 * resnorm_cap entries; results[nrhs]).  Replaces the back-to-back gmres! calls for several incident directions
 * (tests/plasma_example.jl:160-176): each right-hand side keeps its own Krylov basis, Hessenberg matrix and stopping
 * test -- its iterates are those of lsfc_gmres on that right-hand side alone -- but every Arnoldi step applies the
 * operator to all unconverged right-hand sides in one batched pass (see lsfc_apply_batch).  With precond =
 * lsfc_precond_callback and precond_on_device = 1 the right-hand sides meet at the preconditioner as well: one
 * lsfc_precond_apply_batch-style group sweep over the Krylov vectors of all unconverged right-hand sides per step.  Any
 * other callback (host, or the caller's own device callback) is invoked for one right-hand side at a time, in the order of
 * the right-hand sides.  No host threads: everything, the callback included, runs on the calling thread, and the groups of
 * the batched passes are formed in the order of the right-hand sides, the same in every run.  Returns LSFC_OK even if some
 * right-hand side hit maxiter: check results[j].converged.  Device memory: nrhs * (restart + 2) vectors of N complex for the duration of the call (checked
 * against the free memory up front: LSFC_ENOMEM with the figures; released on return). */
int lsfc_gmres_batch(lsfc_plan* plan, double* x, const double* b, int64_t nrhs, const lsfc_gmres_opts* opts,
                     double* resnorm, int64_t resnorm_cap, lsfc_gmres_result* results, int memspace);

/* ---- BiCGStab(l) ------------------------------------------------------------ */

/* Replaces IterativeSolvers.bicgstabl!(x, A, b, l; Pl, max_mv_products, abstol, reltol, log=true): the short-recurrence
 * alternative to lsfc_gmres for grids whose Krylov basis does not fit.  Left-preconditioned (it solves Pl^-1 A x = Pl^-1 b;
 * the residuals below are preconditioned residuals).  One cycle = l BiCG steps (2 operator applications each) and one
 * minimal-residual step over the l + 1 residual vectors; result->iters counts cycles, resnorm has one entry per cycle
 * (||rs[0]|| after the cycle, computed from the vector), result->mvps counts operator applications (1 for the initial
 * residual, 0 with initially_zero, 2 l per cycle).  The cycle loop runs while the residual is above
 * max(reltol * ||Pl^-1 r0||, abstol) and mvps < max_mv_products, so mvps may pass the cap by less than one cycle.
 * DEPARTURE from upstream: the shadow residual is not rand -- it is the preconditioned initial residual, or r_shadow.
 * Two solves of the same input are bitwise equal.
 * Memory rule: 2 l + 3 work vectors of N complex (rs[0..l], us[0..l], the shadow residual) for the duration of the call,
 * whatever the iteration count (5 at l = 1, 7 at l = 2); with LSFC_MEM_HOST the staged x and b on top, as in lsfc_gmres.
 * Checked against the free device memory before anything is allocated: LSFC_ENOMEM with the figures.
 * Exhausted Krylov space: a cycle whose Gram matrix has G[0,0] = ||rs[0]||^2 <= tol^2 records sqrt(G[0,0]) and stops
 * converged without the minimal-residual solve.
 * Breakdown: a rho, sigma or gamma that is zero where it divides, or not finite, ends the solve; every update whose scalar
 * is affected is skipped on the device, so x stays the last finite iterate and rs[0] its residual.  If that residual is
 * already within the tolerance the solve has converged; otherwise LSFC_ENOTCONV, and lsfc_last_error names the scalar and
 * the cycle.  LSFC_ENOTCONV also when max_mv_products is reached (x still updated).
 * LSFC_EINVAL, before any device call: NULL opts, l outside 1..8, a non-zero reserved word, a bad memspace, NULL plan, x,
 * b or result, a distributed or multi-device plan (lsfc_bicgstabl_multi solves on a multi-device plan).
 * Out of scope: multi-process distributed plans. */
typedef struct lsfc_bicgstabl_opts {
    int     l;               /* 1..8; IterativeSolvers' default is 2                                   */
    int64_t max_mv_products; /* <=0: N                                                                 */
    double  reltol;          /* <0: sqrt(eps)                                                          */
    double  abstol;          /* default 0                                                              */
    int     initially_zero;  /* skip the initial A*x0 (x0 == 0)                                        */
    lsfc_precond_fn precond; void* precond_user;  /* NULL: Identity(); as in lsfc_gmres_opts           */
    int     precond_on_device; /* as in lsfc_gmres_opts; lsfc_precond_callback with 1: no host code inside the BiCG part */
    const double* r_shadow;  /* NULL: the preconditioned initial residual; else N complex in `memspace` */
    int     reserved[4];     /* zero */
} lsfc_bicgstabl_opts;

int lsfc_bicgstabl(lsfc_plan* plan, double* x, const double* b, const lsfc_bicgstabl_opts* opts,
                   double* resnorm, int64_t resnorm_cap, lsfc_gmres_result* result, int memspace);

/* lsfc_bicgstabl on a single-process MULTI-DEVICE plan (lsfc_plan_create_gv3d_multi), under the rules lsfc_gmres has there: x, b
 * and opts->r_shadow are LSFC_MEM_HOST vectors of the full size N, scattered over the ranks' z slabs (x is gathered back on
 * return), and the preconditioner is a host callback, called on the calling thread with the WHOLE vector (the slabs are gathered
 * into a pinned host vector and scattered back) at the places where lsfc_bicgstabl preconditions.  A separate entry point, so
 * that what lsfc_bicgstabl does with such a plan (LSFC_EINVAL) does not change.  Every rank keeps its slab of the 2 l + 3 work
 * vectors and its own scalars; a sum is completed in two levels -- each rank reduces its block partials to a rank sum, copies
 * it into a small table on every other rank (event-ordered device copies: (2 l + 2) reductions of P (P - 1) copies per cycle),
 * and the kernel that consumes the sum adds the P entries in rank order.  So every rank forms every scalar from the same
 * numbers in the same order, the host reads the scalars of rank 0 once per cycle, and every documented property of
 * lsfc_bicgstabl carries over unchanged: iteration semantics, history, mvps, tolerances, the exhausted-space exit, the breakdown
 * rules and messages, the shadow-residual departure, bitwise repeatability; one rank on an operator whose apply is bitwise the
 * identity gives the bits of lsfc_bicgstabl on a single-device plan.
 * Memory rule, checked before anything is allocated: each rank needs 2 l + 3 work vectors of N / P complex plus its staged
 * x and b slabs, against the free memory of ITS device (ranks that share a device are summed); LSFC_ENOMEM names the device
 * and gives the figures.
 * LSFC_EINVAL, before any device call: the checks of lsfc_bicgstabl on opts and the pointers; a plan that is not a multi-device
 * one (a single-device plan: lsfc_bicgstabl solves there; a multi-process distributed plan, lsfc_dist_plan_create_gv3d: not
 * offered); LSFC_MEM_DEVICE; precond_on_device = 1 ("a multi-device plan takes a host preconditioner callback").
 * Out of scope: a batched form, multi-process plans, a device preconditioner, the transposed / adjoint operator and complex nu
 * on multi-device plans. */
int lsfc_bicgstabl_multi(lsfc_plan* plan, double* x, const double* b, const lsfc_bicgstabl_opts* opts,
                         double* resnorm, int64_t resnorm_cap, lsfc_gmres_result* result, int memspace);

/* How a member of lsfc_bicgstabl_batch ended (status[2 j]); 2..7 name the scalar of a breakdown. */
#define LSFC_BICG_CONVERGED 0   /* within its tolerance (an exhausted Krylov space included)          */
#define LSFC_BICG_MAX_MV    1   /* max_mv_products reached                                            */
#define LSFC_BICG_RHO       2   /* rho is not finite                                                  */
#define LSFC_BICG_SIGMA     3   /* sigma is zero or not finite                                        */
#define LSFC_BICG_BETA      4   /* beta = rho / sigma is not finite                                   */
#define LSFC_BICG_ALPHA     5   /* alpha = rho / sigma is not finite                                  */
#define LSFC_BICG_GAMMA     6   /* singular or non-finite Gram matrix of the minimal-residual step    */
#define LSFC_BICG_RESIDUAL  7   /* the residual norm is not finite                                    */

/* nrhs solves of lsfc_bicgstabl in lock step, the BiCGStab(l) form of lsfc_gmres_batch (x, b: nrhs vectors back to back;
 * resnorm: nrhs rows of resnorm_cap entries; results[nrhs]; opts->r_shadow: NULL or nrhs vectors back to back in
 * `memspace`; l, the tolerances, the cap, initially_zero and the preconditioner are shared).  The kernel sequence of a
 * cycle does not depend on the data, so every step of a cycle is ONE launch over the members still running and the host
 * reads the scalars of all of them in one copy per cycle: no host threads.  The operator is applied to the running
 * members in groups (see lsfc_apply_batch); with precond = lsfc_precond_callback and precond_on_device = 1 the
 * preconditioner takes them in lsfc_precond_apply_batch-style group sweeps on the plan's stream; any other callback
 * (host, or the caller's own device callback) is called for one member at a time.
 * Member j has its own tol = max(reltol * ||Pl^-1 r0_j||, abstol) and stopping test.  A member that has converged,
 * broken down or reached max_mv_products leaves the group, its x final; a breakdown in one member does not touch the
 * others.  Member j's iterates, history, iters, mvps and converged are those of lsfc_bicgstabl on that right-hand side
 * alone: bit for bit wherever the batched operator and preconditioner applies are bitwise member-independent (the rocFFT
 * pipelines, objects of lsfc_precond_create, block-tridiagonal objects); on the pruned pipeline with a fused batch pass
 * to the rounding of lsfc_apply_batch.
 * status (may be NULL): 2 * nrhs entries, (LSFC_BICG_* code, cycle) per member; the cycle of the breakdown, else the
 * number of cycles run.
 * Returns LSFC_OK even if some member did not converge (check results[j].converged); lsfc_last_error then names the first
 * such member, its reason and its cycle.  LSFC_EINVAL, before any device call: the checks of lsfc_bicgstabl, nrhs outside
 * 1..64, NULL results (a multi-device plan included: the batched solve is not offered there).  Device memory: nrhs * (2 l + 3) work vectors of N complex, with LSFC_MEM_HOST the staged x and b
 * (2 nrhs vectors) on top, checked before anything is allocated: LSFC_ENOMEM with the figures and the largest nrhs that
 * fits. */
int lsfc_bicgstabl_batch(lsfc_plan* plan, double* x, const double* b, int64_t nrhs, const lsfc_bicgstabl_opts* opts,
                         double* resnorm, int64_t resnorm_cap, lsfc_gmres_result* results, int64_t* status, int memspace);

/* ---- device-resident SparsifyingPreconditioner apply ------------------------ */

/* The reference's preconditioner (src/preconditioner.jl:27-58) holds two sparse matrices and a sparse LU:
 *     SparsifyingPreconditioner(Msp, As):  MspInv = lu(Msp)          (:35, UMFPACK)
 *     ldiv!(P, b):  b[:] = MspInv \ (As * b)                          (:132-170)
 * lsfc_precond keeps As and the LU factors on the device and applies v <- Msp^{-1} (As v) there (CSR SpMV, two
 * level-scheduled sparse triangular solves replayed from one hipGraph), so the Krylov vector does not cross PCIe.
 * The factorisation stays with the caller (host): with (Rs .* Msp)[p, q] = L U pass
 *     L, U         CSR, 0-based, diagonals stored (L's unit diagonal included), values interleaved complex
 *     row_gather   k -> row of Msp that becomes row k of L U   (Julia: F.p .- 1;  NULL = identity)
 *     col_scatter  k -> column of Msp behind column k of L U   (Julia: F.q .- 1;  NULL = identity)
 *     row_scale    Rs (Julia: F.Rs), NULL = ones
 * As: CSR, 0-based, N rows.  All index arrays are int64_t.
 * An lsfc_precond owns its work vectors: applies on one object are serialised by the stream they are enqueued on;
 * do not apply the same object from two streams or threads at once. */
typedef struct lsfc_precond lsfc_precond;
int lsfc_precond_create(lsfc_precond** out, int64_t N,
                        const int64_t* As_rowptr, const int64_t* As_col, const double* As_val,
                        const int64_t* L_rowptr, const int64_t* L_col, const double* L_val,
                        const int64_t* U_rowptr, const int64_t* U_col, const double* U_val,
                        const int64_t* row_gather, const int64_t* col_scatter, const double* row_scale, int device);
int lsfc_precond_destroy(lsfc_precond* pc);
/* hipStream_t the apply is enqueued on (NULL = legacy default stream); use the plan's stream under lsfc_gmres */
int lsfc_precond_set_stream(lsfc_precond* pc, void* stream);
/* v <- Msp^{-1} (As v); LSFC_MEM_DEVICE: stream-ordered, returns without synchronising */
int lsfc_precond_apply(lsfc_precond* pc, double* v, int memspace);
/* nrhs vectors back to back (v + j*N), each overwritten with Msp^{-1} (As v_j).  Block-tridiagonal objects: groups of
 * up to 8 go through ONE sweep that reads every S_k^{-1} once per group.  Objects of lsfc_precond_create: member by member.
 * The bits of a vector's result do not depend on nrhs, on its place among the others or on what the others hold; on an
 * object of lsfc_precond_create they are those of lsfc_precond_apply.  Work buffers (three of R*N complex for the largest
 * group R so far, plus the sweep's own) are allocated on first use.  LSFC_MEM_HOST: staged through device memory,
 * synchronises; LSFC_MEM_DEVICE: stream-ordered.  LSFC_EINVAL (before any device call): NULL argument, nrhs < 1, bad memspace. */
int lsfc_precond_apply_batch(lsfc_precond* pc, double* v, int64_t nrhs, int memspace);
/* out[0] group sweeps enqueued since creation, out[1] vectors that went through them, out[2] largest group so far,
 * out[3] bytes of batch work buffers.  All 0 on an object of lsfc_precond_create. */
int lsfc_precond_batch_info(const lsfc_precond* pc, int64_t out[4]);
/* lsfc_precond_fn for lsfc_gmres_opts: precond = lsfc_precond_callback, precond_user = pc, precond_on_device = 1 */
int lsfc_precond_callback(void* user, double* v, int64_t n);
/* dependency levels of the two triangular solves and kernel launches captured in the graph */
int lsfc_precond_stats(const lsfc_precond* pc, int64_t* levels_L, int64_t* levels_U, int64_t* launches);
/* What the launch schedule of one triangular solve reached (factor 0 = L, 1 = U), fixed at lsfc_precond_create.
 * The rows of a factor are sorted by dependency level and the levels cut into four kinds of segments:
 *     out[0..3]  levels launched on their own (more than 32 rows -- LSFC_PRECOND_NARROW -- or more than 8192 entries) at
 *                8, 16, 32, 64 lanes per row
 *     out[4]     chain segments: runs of narrow, light levels walked by one workgroup
 *     out[5]     groups of several levels (<= 16 rows, coupled through a dense block) inside the chain segments
 *     out[6]     heavy groups: such a group with more than 8192 entries, launched on its own between chain segments
 *     out[7]     dense-run pieces: >= 96 rows in consecutive levels of <= 4 rows, cut into pieces of <= 1024 rows
 *     out[8]     rows of the largest dense-run piece (0 if none)
 *     out[9]     rows of the smallest dense-run piece (0 if none)
 * LSFC_EINVAL: NULL pc or out, factor not 0 or 1. */
int lsfc_precond_schedule(const lsfc_precond* pc, int factor, int64_t out[10]);

/* The same object factorised ON THE DEVICE, in place of the host's lu(Msp) (src/preconditioner.jl:35;
 * examples/example3D.jl:57-68 build As, AG, Msp and call SparsifyingPreconditioner(Msp, As)).  As and Msp share one
 * pattern, as lsfc_sparsify_build returns it (CSR, 0-based, columns ascending, values interleaved complex); with the
 * slowest grid axis as block index Msp is block tridiagonal: nblocks blocks of b = N / nblocks rows.  Exact block
 * elimination S_0 = D_0, S_k = D_k - L_k S_{k-1}^{-1} U_{k-1} with the explicit inverses S_k^{-1} kept dense
 * (nblocks * b^2 * 16 bytes of device memory); the apply is As v, then 2 nblocks - 1 dense b x b products.
 * memspace: LSFC_MEM_HOST or LSFC_MEM_DEVICE for the four arrays (the device output of lsfc_sparsify_build is taken as it is).
 * The Schur blocks are inverted WITHOUT pivoting (they are well conditioned: |pivot| / max|S_k| >= 0.5 observed); every
 * pivot is monitored and |pivot| / max|S_k| < 1e-8 (or a pivot that is not a number) is a breakdown: LSFC_EINVAL with
 * block and row in lsfc_last_error, no object is returned.
 * LSFC_EINVAL: NULL pointer, N not divisible by nblocks, a row that is not sorted CSR, an entry outside the three block
 * diagonals (the row is named), breakdown.  LSFC_ENOMEM (decided from N and nblocks alone, before an array is read or
 * anything is allocated): inverses plus work space exceed the free device memory; the message has the figures.
 * Two factorisations of the same input are bitwise equal. */
int lsfc_precond_create_blocktri(lsfc_precond** out, int64_t N, int64_t nblocks, const int64_t* rowptr, const int64_t* col,
                                 const double* As_val, const double* Msp_val, int memspace, int device);
/* lsfc_sparsify_build into device memory, then lsfc_precond_create_blocktri with nblocks = the slowest axis (m in 2D,
 * l in 3D), on the plan's device: examples/example3D.jl:57-68 in one call.  Restrictions of lsfc_sparsify_build. */
int lsfc_precond_create_from_plan(lsfc_precond** out, lsfc_plan* plan);
/* The same two constructors with the storage of the inverses chosen: the functions above are the LSFC_PRECOND_INV_F64 case.
 * LSFC_PRECOND_INV_F32 keeps every S_k^{-1} as interleaved float pairs, nblocks * b^2 * 8 bytes: half the memory rule and
 * half the bytes an apply reads.  The elimination is the fp64 one, unchanged: S_k^{-1} is computed in an fp64 work block
 * (the Schur update of block k + 1 reads it there), then rounded ONCE to nearest-even and stored, so the stored blocks
 * are bit for bit the fp64 object's blocks cast to float, and min_pivot_ratio is that of the fp64 object.  The applies
 * widen every entry to fp64 on load and sum in fp64 in the fp64 object's order.  The object is a fixed linear operator
 * about 1e-7 (relative) away from the fp64 one: left-preconditioned GMRES solves A x = b to the same tolerance with it.
 * Work space during the factorisation: two more fp64 blocks (2 b^2 16 bytes).  LSFC_ENOMEM as above, decided from N,
 * nblocks and the precision alone; the message names the precision.
 * LSFC_EINVAL (before any device call): inverse_precision is neither constant. */
#define LSFC_PRECOND_INV_F64 0   /* as today */
#define LSFC_PRECOND_INV_F32 1   /* S_k^{-1} stored as interleaved float pairs */
int lsfc_precond_create_blocktri_prec(lsfc_precond** out, int64_t N, int64_t nblocks, const int64_t* rowptr, const int64_t* col,
                                      const double* As_val, const double* Msp_val, int memspace, int device, int inverse_precision);
int lsfc_precond_create_from_plan_prec(lsfc_precond** out, lsfc_plan* plan, int inverse_precision);
/* precision: LSFC_PRECOND_INV_F64 or _F32, as the object was made.  LSFC_EINVAL on an object of lsfc_precond_create. */
int lsfc_precond_inverse_precision(const lsfc_precond* pc, int* precision);
/* The same two constructors with options.  opts == NULL is the LSFC_PRECOND_INV_F64 / LSFC_PRECOND_PIVOT_NONE case, and the
 * four constructors above are calls of these two.  pivoting:
 *     LSFC_PRECOND_PIVOT_NONE     the inversion without pivoting described above (the default)
 *     LSFC_PRECOND_PIVOT_PARTIAL  partial ROW pivoting inside every Schur block (never across blocks): at elimination step p
 *                                 the pivot is the row among p .. b-1 with the largest x*x + y*y (fp64) in column p, the
 *                                 lowest such row on a tie.  Gauss-Jordan with interchanges inverts Pi_k S_k; the columns
 *                                 are put back once, so the stored block is S_k^{-1} itself and the applies, the float
 *                                 storage and the memory of the inverses are as without pivoting.  Work space during the
 *                                 factorisation: one more panel (b * 32 * 16 bytes); the pivots are kept (nblocks * b * 4 bytes).
 *     LSFC_PRECOND_PIVOT_AUTO     without pivoting first; after a breakdown the whole factorisation again with _PARTIAL:
 *                                 the object is bit for bit the _NONE object or the _PARTIAL object of the same input
 * The monitor is the same: min_pivot_ratio is the smallest chosen |pivot| / max|S_k|; a chosen pivot below 1e-8 (or not a
 * number) under _PARTIAL means the block is singular to working precision: LSFC_EINVAL with block and row, no object.
 * LSFC_ENOMEM as above, from N, nblocks and the options alone (_AUTO counts as _PARTIAL).
 * LSFC_EINVAL (before any device call): unknown inverse_precision or pivoting, a reserved word that is not zero. */
#define LSFC_PRECOND_PIVOT_NONE 0
#define LSFC_PRECOND_PIVOT_PARTIAL 1
#define LSFC_PRECOND_PIVOT_AUTO 2
typedef struct lsfc_blocktri_opts { int inverse_precision; int pivoting; int reserved[6]; } lsfc_blocktri_opts; /* reserved: zero */
int lsfc_precond_create_blocktri_opts(lsfc_precond** out, int64_t N, int64_t nblocks, const int64_t* rowptr, const int64_t* col,
                                      const double* As_val, const double* Msp_val, int memspace, int device, const lsfc_blocktri_opts* opts);
int lsfc_precond_create_from_plan_opts(lsfc_precond** out, lsfc_plan* plan, const lsfc_blocktri_opts* opts);
/* perm[i] = row of S_k that became pivot row i (identity on an object factorised without pivoting); b entries.
 * LSFC_EINVAL: object made by lsfc_precond_create, k out of range, capacity < b. */
int lsfc_precond_blocktri_get_pivots(const lsfc_precond* pc, int64_t k, int64_t* perm, int64_t capacity);
/* out: blocks, block size b, bytes of the stored inverses (nblocks b^2 16, or 8 at float storage), kernel launches per apply, factorisation time in
 * microseconds, 1 if the stored blocks come from the pivoted elimination (LSFC_PRECOND_PIVOT_PARTIAL, or _AUTO after it fell
 * back), else 0; min_pivot_ratio (may be NULL): smallest |pivot| / max|S_k| met.
 * LSFC_EINVAL on an object made by lsfc_precond_create. */
int lsfc_precond_blocktri_info(const lsfc_precond* pc, int64_t out[6], double* min_pivot_ratio);
/* Debug / test access in the spirit of lsfc_plan_get_symbol: S_k^{-1} (b x b, column-major) to the host, as stored
 * (at float storage: the stored float pairs widened to double).
 * LSFC_EINVAL: object made by lsfc_precond_create, k out of range, capacity_complex < b^2. */
int lsfc_precond_blocktri_get_block(const lsfc_precond* pc, int64_t k, double* out, int64_t capacity_complex);
/* On such an object, at either storage, lsfc_precond_apply / _apply_batch / _batch_info / _callback / _set_stream /
 * _destroy work as on any other, and lsfc_gmres_batch groups its members' applies as before; lsfc_precond_stats
 * returns nblocks, nblocks and the launch count; lsfc_precond_schedule returns LSFC_EINVAL (there are no levels). */

/* The transposed and the adjoint preconditioner of a block-tridiagonal object.  P = Msp^-1 As approximates inv(M), so
 *     P^T = As^T Msp^-T  approximates inv(M^T)      and      P^H v = conj(P^T conj(v))  approximates inv(M^H).
 * Msp^-T is applied from the SAME stored inverses S_k^-1 (no second copy, no second factorisation) by
 *     forward    z_k = S_k^-T (w_k - U_{k-1}^T z_{k-1})                  k = 0 .. K-1
 *     backward   x_{K-1} = z_{K-1},  x_k = z_k - S_k^-T (L_{k+1}^T x_{k+1})   k = K-2 .. 0
 * and As^T follows the sweeps (under N the SpMV comes first).  An apply reads the bytes the N apply reads.
 *
 * The op is state of the object (default LSFC_OP_N), as it is of a plan.  It is READ by lsfc_precond_apply,
 * lsfc_precond_apply_batch, lsfc_precond_callback and by the group sweeps inside lsfc_gmres_batch and
 * lsfc_bicgstabl_batch.  Everything else keeps describing the N object: lsfc_precond_stats, _blocktri_info, _get_block,
 * _get_pivots, _batch_info and _inverse_precision.
 * The first lsfc_precond_set_op(T | H) builds the CSR of Msp^T and As^T on the device (deterministic: two objects of one
 * input apply bitwise alike); it synchronises and allocates, so it must not run inside a stream capture.  *table_bytes
 * (may be NULL) is the size of those tables, 0 on an object that never left N; such an object allocates nothing more and
 * launches exactly what it launched before this call existed.
 * LSFC_EINVAL, before any device call: NULL pc; op outside 0..2; T | H on an object of lsfc_precond_create (the transposed
 * apply needs a block-tridiagonal object; the transposed level-scheduled solves are not offered). */
int lsfc_precond_set_op(lsfc_precond* pc, int op);     /* LSFC_OP_N (default) | LSFC_OP_T | LSFC_OP_H */
int lsfc_precond_get_op(const lsfc_precond* pc, int* op, int64_t* table_bytes /* may be NULL */);

/* ---- assembly of the sparsifying matrices (As, As*G, Msp) ------------------- */

/* The reference builds the two matrices of SparsifyingPreconditioner(Msp, As) with buildSparseA / buildSparseAG
 * (src/SparsifyingMatrix2D.jl:351-438, :806-884, Conv variants :441-532, :888-966) and buildSparseA3DConv /
 * buildSparseAG3DConv (src/SparsifyingMatrix3D.jl:1410-1918), and the caller forms Msp = As + k^2 AG diag(nu)
 * (examples/example.jl:67, examples/example3D.jl:61).  Every grid point belongs to one stencil class (2D: 9, 3D: 27;
 * class numbers in the reference's order, DESIGN.md "Sparsifying matrices"); class c has a_c = U[:, end]' of
 * svd(G[S_c, complement of S_c]) for its sample sources S_c, stamped on the rows of its class (As) together with
 * a_c G[S_c, S_c] (AG, with the reference's entriesSparseG* source order).
 * Matrices: CSR, 0-based, columns ascending in every row, every stencil entry stored (also an exact 0), values
 * interleaved complex.  The three matrices share one pattern.
 * Phase: U[:, end] is defined up to a unit complex factor; a_c is scaled so that its entry of largest modulus (the
 * first one in the reference's stencil order on ties) is real and positive.  As and AG rows carry the same factor,
 * so Msp^{-1} As does not depend on it. */

/* Pattern of As / AG / Msp (identical) for a 2D (l == 1) or 3D grid: pure host arithmetic, no device.  nnz (out);
 * rowptr[N+1], col[nnz], row_class[N] may each be NULL (query nnz first).  LSFC_EINVAL: an axis < 3, 2D with n or m even. */
int lsfc_sparsify_pattern(int64_t n, int64_t m, int64_t l, int64_t* nnz, int64_t* rowptr, int64_t* col, int64_t* row_class);

/* buildSparseA*Conv / buildSparseAG*Conv from the plan's own discrete kernel, and Msp = As + omega^2 AG diag(nu).
 * Any value array may be NULL.  sigma (NULL or nclass*3): sigma_max, sigma_second_smallest, sigma_min per class.
 * memspace: LSFC_MEM_HOST or LSFC_MEM_DEVICE for all array arguments.
 * The rows are those of the plan's kernel (lsfc_sample_sources, no nu): a 2D trapezoidal plan gives the directly
 * sampled sampleG rows of buildSparseA / buildSparseAG, Greengard-Vico plans the Conv variants.  nu and omega are the
 * plan's.  LSFC_EINVAL: NULL, distributed or multi-device plan, unsupported grid (as lsfc_sparsify_pattern, or fewer
 * than twice as many points as a stencil has sources), an array that is detectably not in `memspace`, a kernel that is
 * not even along every axis (lsfc_sample_sources above: the message names axis and deviation, nothing is written;
 * lsfc_precond_create_from_plan* pass the refusal on).  The op of the plan (lsfc_plan_set_op) is neither read nor changed.
 * sigma: the three values are Rayleigh quotients |G_S^H u| of the eigenvectors of the class's Gram matrix, summed with
 * compensation from the rows themselves; they agree with an SVD of the rows to a few eps sigma_max, also where
 * sigma_min / sigma_max is 1e-5 (the eigenvalues of the Gram matrix would be off by eps sigma_max^2 / sigma there).
 * Device memory: about 0.3 MB of tables plus, for LSFC_MEM_HOST, staging for the requested arrays. */
int lsfc_sparsify_build(lsfc_plan* plan, int64_t* rowptr, int64_t* col, double* As_val, double* AG_val,
                        double* Msp_val, double* sigma, int memspace);

/* ---- off-grid sources and receivers ------------------------------------------- */

/* The reference's drivers build the incident field on the host and stop at the total field on the grid
 * (examples/example3D.jl:46-50, :78-81; examples/example.jl:40-44, :85-99).  lsfc_receivers is what comes before and after:
 * the dense nrecv x N sampling operator R between grid vectors and nrecv receivers off the grid, never stored, with its
 * transpose and its adjoint.  Grid: dims = (n, m[, l]) points x_i = origin + h (ix, iy[, iz]), x fastest; k > 0 real.  The
 * rows are the reference's free-space Green's function weighted by h^d (src/FastConvolution3D.jl:188,
 * src/FastConvolution.jl:268), or its far-field limit:
 *     LSFC_RECV_POINTS    3D   R[r,i] = h^3 e^{ik|p_r - x_i|} / (4 pi |p_r - x_i|)            coords: nrecv points p_r
 *                         2D   R[r,i] = h^2 (i/4) (J0 + i Y0)(k |p_r - x_i|)
 *     LSFC_RECV_FARFIELD  3D   R[r,i] = (h^3 / 4 pi) e^{-ik theta_r . x_i}                   coords: nrecv unit vectors theta_r
 *                         2D   R[r,i] = h^2 e^{i pi/4} / sqrt(8 pi k)  e^{-ik theta_r . x_i}
 * so that R_points(rho theta) q -> e^{ik rho} / rho^((d-1)/2) R_far(theta) q as rho -> infinity.
 * lsfc_receivers_apply works on nrhs vectors stored back to back:
 *     LSFC_OP_N   out_j[r] = sum_i R[r,i] in_j[i]             in: nrhs * N,      out: nrhs * nrecv
 *     LSFC_OP_T   out_j[i] = sum_r R[r,i] in_j[r]             in: nrhs * nrecv,  out: nrhs * N      (the field of point sources)
 *     LSFC_OP_H   out_j[i] = sum_r conj(R[r,i]) in_j[r]                                             (far field: plane waves)
 * `out` must not alias `in`.  With a plan the medium is fused into the operation: N becomes -omega^2 R (nu .* u), the
 * scattered field at the receivers for the total field u; T becomes -omega^2 nu .* (R^T w) and H becomes
 * -omega^2 conj(nu) .* (R^H w) -- the conjugation is outermost, the rule of lsfc_plan_set_op.  nu and omega are the plan's
 * (real or complex nu, read on the device at the time the kernels run); the plan's op is neither read nor changed.
 * Sums: a receiver's sum over the grid is the two-stage fixed-order reduction the Krylov kernels use, a grid point's sum over
 * the receivers runs r = 0 .. nrecv-1.  Two applies of the same input give the same bits, and the bits of one receiver's
 * (grid point's) or one member's result do not depend on nrecv, on nrhs, on its place among the others or on what they hold.
 * Members go through the kernels in groups of up to 8; the kernel function is evaluated once per (point, receiver) and group.
 * Work buffers (block partials, staging of host vectors) belong to the object and grow on first use: do not apply one object
 * from two streams or threads at once.  LSFC_MEM_DEVICE: stream-ordered on the object's stream (lsfc_receivers_set_stream,
 * NULL = the legacy default stream), returns without synchronising.  LSFC_MEM_HOST: staged through device memory, synchronises.
 * LSFC_EINVAL, before any device call, lsfc_last_error names the cause: a NULL argument; ndim not 2 or 3; a dimension < 1 (or
 * 2^31 grid points and more); h <= 0 or k <= 0; nrecv < 1; nrhs < 1; an unknown kind, op or memspace; a far-field direction
 * whose norm differs from 1 by more than 1e-12; a point receiver closer than 1e-8 h to a grid point (the nearest grid point
 * is found by rounding; the message names the receiver's index); a plan whose lsfc_plan_size is not N or whose device differs;
 * a distributed, simulated-rank or multi-device plan ("not available on ...").
 * Out of scope: multi-device and multi-process plans; receivers on grid points (the kernel is singular there); quadrature
 * corrections for receivers inside the support of nu -- the sum is the plain trapezoidal rule, spectrally accurate for
 * receivers at a distance from a smooth, compactly supported nu; NUFFT-accelerated evaluation. */
typedef struct lsfc_receivers lsfc_receivers;
#define LSFC_RECV_POINTS   0
#define LSFC_RECV_FARFIELD 1
/* coords: nrecv * ndim doubles on the host (copied) */
int lsfc_receivers_create(lsfc_receivers** out, int ndim, const int64_t dims[3], const double origin[3], double h, double k,
                          int kind, const double* coords, int64_t nrecv, int device);
int lsfc_receivers_destroy(lsfc_receivers* rc);
int lsfc_receivers_set_stream(lsfc_receivers* rc, void* hip_stream);
/* op: LSFC_OP_N | LSFC_OP_T | LSFC_OP_H; plan may be NULL */
int lsfc_receivers_apply(lsfc_receivers* rc, lsfc_plan* plan, const double* in, double* out, int64_t nrhs, int op, int memspace);
/* out: N, nrecv, receivers per thread of the forward kernel, receivers per LDS chunk of the T / H kernel, members per group,
 * bytes of the tables (receiver coordinates, or the nrecv (n + m + l) complex far-field factors) */
int lsfc_receivers_info(const lsfc_receivers* rc, int64_t out[6]);

/* ---- linearised scattering: the Born operator J, J^H and the misfit gradient ---- */

/* With M = I + omega^2 G diag(nu), M u_s = u_inc_s and the data d_s = -omega^2 R (nu .* u_s) of lsfc_receivers_apply with a plan,
 * the Frechet derivative of nu -> d and its adjoint are (G symmetric, so that G M^T = M G)
 *     J_s dnu = -omega^2 R M^-T (u_s .* dnu)                                 one M^T solve per source, then the plain R
 *     J^H r   = sum_s -omega^2 conj(u_s .* p_s),   M p_s = R^T conj(r_s)     one M solve per source (reciprocity)
 * J is complex-linear in dnu and holds for a complex nu as it stands; for a real nu the gradient of
 * phi = 1/2 sum_s ||d_s - d_obs_s||^2 is Re(J^H (d - d_obs)).  conj(M)^-1 is none of N / T / H: the conjugations of J^H sit in the
 * two kernel-level entries below, which are usable on their own.  N, device and stream are the plan's; the plan's nu and op are
 * neither read nor changed by them.  Vectors: nrhs members back to back, LSFC_MEM_HOST (staged, synchronises) or LSFC_MEM_DEVICE
 * (stream-ordered on the plan's stream).
 *   lsfc_born_scale   out_j[i] = dnu[i] u_j[i].  dnu: N doubles, or N (re, im) pairs with dnu_is_complex; read once per group of up
 *                     to 8 members.  out may be u.
 *   lsfc_born_image   g[i] = (LSFC_BORN_ACCUMULATE ? g[i] : 0) + sum_j scale conj(u_j[i] p_j[i]), serially in member order j: a
 *                     point's bits depend on the order of the members and on nothing else -- one call of 17 members, calls of
 *                     8 + 8 + 1 with LSFC_BORN_ACCUMULATE and 17 calls of one give the same bits.  LSFC_BORN_REAL: g is N doubles and
 *                     receives the real part, bit for bit that of the complex result (the running real part never reads the
 *                     imaginary one, so g itself carries it from launch to launch).
 * LSFC_EINVAL, before any device call: NULL argument; nrhs < 1; an unknown flag, dnu_is_complex or memspace; a distributed,
 * simulated-rank or multi-device plan ("not available on ..."). */
#define LSFC_BORN_ACCUMULATE 1u
#define LSFC_BORN_REAL       2u
int lsfc_born_scale(lsfc_plan* plan, const double* dnu, int dnu_is_complex, const double* u, double* out, int64_t nrhs, int memspace);
int lsfc_born_image(lsfc_plan* plan, const double* u, const double* p, int64_t nrhs, double scale_re, double scale_im,
                    unsigned flags /* LSFC_BORN_ACCUMULATE | LSFC_BORN_REAL */, double* g, int memspace);

/* The object: a plan, a receivers object and solver options; it owns the background fields U (nsrc x N, on the device), the data
 * and its work vectors, and borrows plan, receivers and preconditioner (they must outlive it).
 * Sequences, each over `chunk` sources at a time with x0 = 0, through lsfc_gmres_batch / lsfc_bicgstabl_batch with LSFC_MEM_DEVICE
 * on the plan's stream (the receivers object and the preconditioner are moved onto that stream):
 *     lsfc_born_set_background   batched solve on M -> U; then the plan-fused R on all of U -> data
 *     lsfc_born_apply, OP_N      lsfc_born_scale (times -omega^2) -> batched solve on M^T -> plain R
 *     lsfc_born_apply, OP_H      conj -> plain R^T -> batched solve on M -> lsfc_born_image with scale -omega^2
 * State: the plan's op and the preconditioner's op are set for the solves (T for OP_N, N otherwise) and PUT BACK TO WHAT THEY WERE
 * on every way out, errors included.
 * Preconditioner: it must be able to follow.  A block-tridiagonal object serves both directions; an object of lsfc_precond_create
 * (host LU, no transposed apply) is accepted for OP_H and the background, and OP_N with it is LSFC_EINVAL naming the reason.
 * Symmetry: lsfc_born_create runs the symmetry check of lsfc_plan_set_op(T); a plan whose defect is above 1e-10 fails with that
 * message.
 * Memory rule, checked by lsfc_born_set_background before anything is allocated: nsrc N 16 B for U; per member of a chunk the
 * solver's vectors (restart + 2, or 2 l + 3 for BiCGStab(l)) and two work vectors; one more work vector (staging of host dnu / g).
 * LSFC_ENOMEM gives the figures and the largest chunk / nsrc that would fit.  chunk <= 0: the largest that fits, at most 64.
 * Non-convergence: a source that does not converge does not stop the others; the outputs are written, the call returns
 * LSFC_ENOTCONV, lsfc_last_error names the first such source and its stage, lsfc_born_info has every source's result.
 * Repeatability: two calls with the same input give the same bits.
 * LSFC_EINVAL, before any device call, lsfc_last_error names the cause: a NULL argument; a non-zero reserved word; an unknown
 * solver, op or flag; l outside 1..8; chunk > 64; LSFC_OP_T; LSFC_BORN_REAL with OP_N; apply, fields or data before
 * lsfc_born_set_background; receivers whose N or device differ from the plan's; a distributed, simulated-rank or multi-device plan.
 * Out of scope: multi-device and multi-process plans; warm starts and recycled Krylov spaces across sources or calls;
 * regularisation, line searches and an optimiser; the second-order adjoint; receivers inside the support of nu; per-source
 * receiver sets. */
typedef struct lsfc_born lsfc_born;
#define LSFC_BORN_GMRES     0
#define LSFC_BORN_BICGSTABL 1
typedef struct lsfc_born_opts {
    int solver;            /* LSFC_BORN_GMRES | LSFC_BORN_BICGSTABL */
    int restart, l;        /* as lsfc_gmres_opts / lsfc_bicgstabl_opts */
    int64_t maxiter;       /* GMRES iterations / BiCGStab(l) max_mv_products; <= 0: N */
    double reltol, abstol; /* reltol < 0: sqrt(eps) */
    lsfc_precond* precond; /* NULL or a library object, applied on the device in group sweeps */
    int64_t chunk;         /* sources solved in lock step; <= 0: the largest that fits, at most 64 */
    int reserved[6];       /* zero */
} lsfc_born_opts;
int lsfc_born_create(lsfc_born** out, lsfc_plan* plan, lsfc_receivers* rc, const lsfc_born_opts* opts);
int lsfc_born_destroy(lsfc_born* b);
/* solves M u_s = u_inc_s for s < nsrc (u_inc: nsrc * N complex), keeps U on the device, forms d_s = -omega^2 R (nu .* u_s); call
 * again after lsfc_plan_set_nu* */
int lsfc_born_set_background(lsfc_born* b, const double* u_inc, int64_t nsrc, int memspace);
int lsfc_born_fields(const lsfc_born* b, const double** u_dev, int64_t* nsrc);       /* device pointer, nsrc * N complex */
int lsfc_born_data(lsfc_born* b, double* d, int memspace);                           /* nsrc * nrecv complex */
/* LSFC_OP_N: dnu (N doubles, or N complex with in_is_complex) -> dd (nsrc * nrecv).  LSFC_OP_H: r (nsrc * nrecv complex) -> g
 * (N complex; N doubles = Re with LSFC_BORN_REAL).  LSFC_OP_T is refused. */
int lsfc_born_apply(lsfc_born* b, const double* in, int in_is_complex, double* out, int op, unsigned flags, int memspace);
/* out: N, nrecv, nsrc, chunk, solver, bytes of device memory held, batched solves of the last call, operator applications of the
 * last call; last (may be NULL): nsrc results of the last call's solves */
int lsfc_born_info(const lsfc_born* b, int64_t out[8], lsfc_gmres_result* last /* nsrc entries, may be NULL */);

/* Reciprocal mode: J and J^H without solves.  Every right-hand side of the solves above lies in a small fixed space: the adjoint
 * sources R^T conj(r_s) span at most nrecv dimensions, and the M^T solves of J are only ever seen through R.  With the receiver
 * fields
 *     V = M^-1 R^T        (N x nrecv; column r is the field of receiver r used as a source: nrecv ordinary solves on M)
 * and R M^-T = V^T the formulas above become contractions of the stored U and V:
 *     (J dnu)[s, r] = -omega^2 sum_i dnu[i] u_s[i] v_r[i]
 *     (J^H r)[i]    = -omega^2 sum_s conj(u_s[i]) sum_r conj(v_r[i]) r[s, r]
 * Only transposes are used; nu may be complex.  Both sides contract the same U and V, so J and J^H are adjoint to rounding whatever
 * the solver tolerance.
 * Cost: nrecv solves per medium (every lsfc_born_set_background) against nsrc solves per apply in the adjoint-state mode above;
 * an apply is then nsrc nrecv complex multiply-adds per grid point over nsrc + nrecv streamed vectors.  Reciprocal mode pays when
 * (applies per medium) x nsrc > nrecv; the adjoint-state mode stays the right one for a single gradient with many receivers.
 *
 * lsfc_born_contract is the kernel-level entry, usable without the object (conventions of lsfc_born_image; u: nsrc x N, v: nrecv x N,
 * members back to back; N, device and stream are the plan's):
 *   LSFC_OP_N   in: N doubles, or N (re, im) pairs with in_is_complex; out[s nrecv + r] = scale sum_i (in[i] u_s[i]) v_r[i].
 *               The sum over the points has two levels: blocks of points (their number and bounds depend on N alone), then the
 *               blocks in order.  out[s, r] is its own chain of multiply-adds: its bits depend on u_s, v_r, in, scale and N, not on
 *               the other members, on nsrc, nrecv or the pair's place.  flags must be 0.  The block partials (8 KB per block and
 *               16 x 16 pairs) are device memory kept with the plan from the first call on.
 *   LSFC_OP_H   in: nsrc x nrecv complex; out[i] = (LSFC_BORN_ACCUMULATE ? out[i] : 0) + conj(scale) sum_s conj(u_s[i]) q_s[i],
 *               q_s[i] = sum_r conj(v_r[i]) in[s, r].  Order: q_s over the receivers in fours, in order; then per group of 16 sources,
 *               in order, t_g = sum of conj(u_s) q_s over s = g, g + 4, g + 8, g + 12 in that order (g = 0..3), the group's value
 *               (t_0 + t_1) + (t_2 + t_3), and conj(scale) times it added to the running out[i].  So one call and two calls cut at a
 *               multiple of 16 sources, the second with LSFC_BORN_ACCUMULATE, give the same bits; other cuts agree to rounding.
 *               LSFC_BORN_REAL: out is N doubles, bit for bit the real part of the complex result.
 *   With conj(scale) in OP_H the two ops are adjoint for any scale.  Two calls give the same bits.  No atomics.
 *   LSFC_EINVAL, before any device call: NULL argument; nsrc or nrecv < 1; an unknown op, flag, in_is_complex or memspace; LSFC_OP_T;
 *   a flag with LSFC_OP_N; a real input with LSFC_OP_H; a distributed, simulated-rank or multi-device plan.
 *
 * The object: lsfc_born_set_mode may be called at any time after lsfc_born_create.  To LSFC_BORN_RECIPROCAL with a background
 * present it solves for V at once, without one the next lsfc_born_set_background does; back to LSFC_BORN_ADJOINT_STATE (the default)
 * releases V.  In reciprocal mode
 *     lsfc_born_set_background   as above, then V: `chunk` receivers at a time, right-hand sides R^T e_r from lsfc_receivers_apply
 *                                (LSFC_OP_T) on rows of the identity, the object's solver, tolerances and preconditioner on M, x0 = 0
 *     lsfc_born_apply, OP_N / H  lsfc_born_contract with scale = -omega^2: no solve, the plan's and the preconditioner's state are not
 *                                touched, LSFC_OK; lsfc_born_info reports 0 solves and 0 operator applications, every source
 *                                converged in 0 iterations.  A host-LU preconditioner (lsfc_precond_create) therefore serves OP_N.
 * Memory rule: reciprocal mode adds nrecv N 16 B for V (and the contraction's block partials, 8 KB x min(1024, N / 4096) per 16 x 16
 * sources x receivers); checked in the same place, before anything is allocated; LSFC_ENOMEM also gives the largest nrecv that fits.
 * Non-convergence: a receiver that does not converge does not stop the others; V is kept, the call returns LSFC_ENOTCONV and
 * lsfc_last_error names the first such receiver and the stage "receiver-field solve on M" (a source that did not converge in the
 * same call is named first); lsfc_born_receiver_info has every receiver's result.
 * LSFC_EINVAL, before any device call, lsfc_last_error names the cause: an unknown mode; a NULL argument; lsfc_born_receiver_fields
 * outside reciprocal mode or before lsfc_born_set_background. */
#define LSFC_BORN_ADJOINT_STATE 0
#define LSFC_BORN_RECIPROCAL    1
int lsfc_born_contract(lsfc_plan* plan, const double* u, int64_t nsrc, const double* v, int64_t nrecv, const double* in, int in_is_complex,
                       double* out, int op, unsigned flags, double scale_re, double scale_im, int memspace);
int lsfc_born_set_mode(lsfc_born* b, int mode);
int lsfc_born_get_mode(const lsfc_born* b, int* mode, int64_t* receiver_field_bytes);
int lsfc_born_receiver_fields(const lsfc_born* b, const double** v_dev, int64_t* nrecv);   /* device pointer, nrecv * N complex */
/* out: nrecv, batched solves, operator applications, first receiver not converged or -1 -- of the last receiver-field solve;
 * per_receiver (may be NULL): nrecv results */
int lsfc_born_receiver_info(const lsfc_born* b, int64_t out[4], lsfc_gmres_result* per_receiver);

/* ---- streams, timing, profiling ------------------------------------------ */

/* Run the plan on a caller-owned hipStream_t (NULL = the legacy default stream). */
int lsfc_plan_set_stream(lsfc_plan* plan, void* hip_stream);
/* Block until all work queued by this plan has finished. */
int lsfc_plan_synchronize(lsfc_plan* plan);
/* Time `reps` back-to-back device-resident applies with HIP events recorded on the
 * plan's stream; *ms_total = elapsed milliseconds for all reps. */
int lsfc_time_apply(lsfc_plan* plan, const double* x_dev, double* y_dev, int reps, double* ms_total);
/* Per-kernel timing of one device-resident apply: HIP events around every stage.
 * names[i] (static strings), ms[i], bytes[i] = algorithmic HBM bytes of stage i. */
int lsfc_profile_apply(lsfc_plan* plan, const double* x_dev, double* y_dev, int reps,
                       int max_stages, const char** names, double* ms, double* bytes, int* nstages);

/* Tuning knobs of the pruned pipeline (benchmarks / autotuning), the run-time form of the LSFC_* environment
 * switches of DESIGN.md section 3: "split_x", "split_s" (re/im-split LDS exchanges of the x / y passes), "split_z",
 * "sym_prefetch", "tw_lds", "z_half" (fused pass: split exchanges, symbol prefetch, LDS-resident stage twiddles,
 * half-tile form), "z_persist" (fused pass: 0 one tile per workgroup, 1-4 persistent pipelined whole tiles (6: handed out by per-XCD tickets), 5 ticketed
 * half tiles, -1 by line length), "xlane" (fused pass, lines with two consecutive stages of equal radix -- 8.8: 512, 1024, 1536 points; 4.4: 128, 192, 320, 384, 640, 1280 --
 * the exchange between them through LDS, 0, or through the lanes of the wavefront, 1; 5 = 1 + row pairs as work items, the default where available; 3 = 1 + mirror symbol values from L2), "ytile_g", "ytile_z" (block-order tile of the y passes), "batch_fuse"
 * (lsfc_apply_batch: 1 one fused pass per group of right-hand sides, 0 member by member, -1 by grid size).  Any other
 * key is LSFC_EINVAL.  Results never depend on them beyond rounding (the forms differ in how twiddles are obtained). */
int lsfc_plan_set_tuning(lsfc_plan* plan, const char* key, int value);
/* Which kernels an apply of nrhs right-hand sides (one group of lsfc_apply_batch, at most LSFC_MAX_BATCH in csrc/pruned.hpp) launches under the plan's present
 * tuning, as text: "pipeline=<lsfc_plan_pipeline>", then for a single-device pruned plan one line per pass in launch order,
 *   <family> L=<line length> SPLIT= FULL= [LINES= WPE=] [FORCED_SPLIT= TG= TZ=] [PREFETCH= ZE= TWL= BATCH= LATE_SYM= TICKETS= XL= PER_MEMBER=]
 * (family: xfwd, yfwd, zfused | zfused_half | zfused_persist | zfused_persist_half, yinv, xinv; the flags are the template
 * arguments of the instantiation, TG x TZ the resolved block-order tile of the y passes, PER_MEMBER=1 a batch that the fused pass
 * runs one right-hand side at a time), and a last line
 *   pitch1= pitch2= sym_rows= sym_hz= ytab=0|1 zmirror=0|1 tile2d= batch=none|fused|per_member
 * (ytab / zmirror: the y-even half of the symbol rows / the even half of every symbol line is stored).  The rocFFT pipelines and
 * distributed or multi-device plans report the pipeline line only.  Pure host arithmetic: nothing is launched.  Sizing as
 * lsfc_plan_get_symbol: *need = bytes including the terminating NUL; buf may be NULL, else capacity >= *need.
 * Requests the dispatcher does not run as asked: z_persist 5 needs >= 1024 points and a multiple of 16 tiles in row pairs, else it
 * runs as 4; 6 needs such tiles too, else it runs as 3; 1-6 run split where whole-complex exchanges of 8 lines exceed the LDS;
 * xlane 3 and 5 need tw_lds (without the table they run through LDS), 5 the ticketed form (else 1); lane exchanges exist
 * in the persistent whole tiles of 128, 192, 256, 320, 384, 512, 640, 768 and 1024 points and in the ticketed half tiles of 1024,
 * 1280, 1536 and 2048 points, XL = 0 elsewhere; tw_lds is dropped where the
 * table does not fit beside the exchange buffer; z_half applies at 1024 and 1536 points with a multiple of 8 tiles only; in 3D
 * the 2048-point line always runs whole-complex half tiles (split_z, sym_prefetch, tw_lds and z_persist 1-4, 6 do not apply), and
 * the 1536-point line runs persistent whole tiles only with z_half = 0; whole-complex exchanges of the one-tile kernels and of
 * the y passes run split from 1280 points on (they exceed the LDS). */
int lsfc_plan_describe_passes(const lsfc_plan* plan, int nrhs, char* buf, int64_t capacity, int64_t* need);

/* ---- device memory helpers for hosts without a HIP binding ---------------- */
int lsfc_device_count(int* count);
int lsfc_malloc(void** dptr, size_t bytes, int device);
int lsfc_free(void* dptr);
int lsfc_memcpy_h2d(void* dst_dev, const void* src_host, size_t bytes);
int lsfc_memcpy_d2h(void* dst_host, const void* src_dev, size_t bytes);
/* Page-lock a long-lived host vector (a Krylov work vector of the caller's solver) so that the host-vector forms of
 * lsfc_apply / lsfc_convolve (mul!(Y, M, b), src/FastConvolution.jl:50-54) move it by DMA instead of through the
 * runtime's staging copies.  Optional: pageable vectors work, at about the same rate on MI355X hosts measured so far.
 * Unregister before the memory is freed. */
int lsfc_host_register(void* ptr, size_t bytes);
int lsfc_host_unregister(void* ptr);
/* Page-locked host memory OWNED BY THE RUNTIME (hipHostMalloc): the preferred way to get DMA-able work vectors -- page-aligned,
 * shares no page with other allocations of the process and is not subject to the kernel's page migration, unlike a registered
 * range of the caller's heap (lsfc_host_register pins user pages in place; ranges that share pages with other heap objects are
 * best avoided, see DESIGN.md "host vectors").  A host that cannot adopt foreign memory for its vectors (Julia can:
 * unsafe_wrap) keeps using pageable vectors or lsfc_host_register. */
int lsfc_host_alloc(void** ptr, size_t bytes);
int lsfc_host_free(void* ptr);

/* ---- slab-distributed 3D operator (one process per GPU, RCCL over xGMI) ---- */

/* 128-byte RCCL unique id: rank 0 calls lsfc_dist_unique_id and ships the bytes to
 * the other ranks with whatever the host already has (torch.distributed, MPI, a file). */
#define LSFC_UNIQUE_ID_BYTES 128
int lsfc_dist_unique_id(unsigned char id[LSFC_UNIQUE_ID_BYTES]);

/* z-slab-partitioned counterpart of lsfc_plan_create_gv3d: this rank owns planes
 * k in [rank*l/nranks, (rank+1)*l/nranks) of nu, x and y.  The padded-grid transform is
 * X-pass -> all-to-all -> Y,Z,symbol,Z^-1,Y^-1 -> all-to-all -> X^-1. */
int lsfc_dist_plan_create_gv3d(lsfc_plan** out, int64_t n, int64_t m, int64_t l, double box, double omega,
                               const double* nu_local, unsigned flags, int device,
                               int rank, int nranks, const unsigned char id[LSFC_UNIQUE_ID_BYTES]);

/* Testing aid for hosts with fewer GPUs than ranks: `nranks` logical ranks as separate plans on ONE device, driven
 * in lock step by lsfc_dist_sim_apply, which performs the two slab exchanges with device-to-device copies instead
 * of RCCL.  Exercises exactly the kernels, layouts and symbol slabs of the multi-GPU path.  x[r], y[r]: host
 * vectors of the local size of rank r.  mode: 0 apply, 1 convolve, 2 convolve with nu. */
int lsfc_dist_sim_plan_create_gv3d(lsfc_plan** out, int64_t n, int64_t m, int64_t l, double box, double omega,
                                   const double* nu_local, unsigned flags, int device, int rank, int nranks);
int lsfc_dist_sim_apply(lsfc_plan** plans, int nranks, const double* const* x, double* const* y, int mode);

/* ---- single-process multi-device 3D operator (ONE host thread drives every GPU) ---- */

/* buildFastConvolution3D for a host that is ONE process -- the reference's own situation (a single Julia process,
 * examples/example3D.jl:54,78) -- on `ndev` devices: rank r = devices[r] owns z planes [r*l/ndev, (r+1)*l/ndev).
 * nu: the full n*m*l contrast (host).  The returned plan behaves like any other with HOST vectors: lsfc_apply,
 * lsfc_convolve, lsfc_apply_batch, lsfc_gmres (host preconditioner callback on the whole vector), lsfc_plan_set_nu,
 * lsfc_profile_apply (x_dev / y_dev ignored), lsfc_plan_synchronize, lsfc_plan_destroy; vectors are scattered over the
 * devices' slabs inside the call and the Krylov basis of lsfc_gmres stays distributed on the devices.  The calling
 * thread enqueues the work of all ranks: x pass -> slab exchange -> y, z, y passes -> slab exchange back -> x pass,
 * in K pipeline chunks with the exchanges on side streams, cross-device ordering by events.
 * Transport of the two exchanges: RCCL grouped ncclSend/ncclRecv over ncclCommInitAll communicators (default when the
 * devices are distinct), or peer-to-peer copies issued by the source rank (environment LSFC_MULTI_TRANSPORT=copy; the
 * only choice when a device is listed more than once, which is how this path is tested on a one-GPU machine).
 * ndev: a power of two dividing l and Lx/8. */
int lsfc_plan_create_gv3d_multi(lsfc_plan** out, int64_t n, int64_t m, int64_t l, double box, double omega,
                                const double* nu, unsigned flags, const int* devices, int ndev);
/* ndev, devices[0..ndev), entries per device slab, name of the exchange transport (any pointer may be NULL) */
int lsfc_multi_info(const lsfc_plan* plan, int* ndev, int* devices, int64_t* local_n, const char** transport);
/* The apply on vectors that already live on the devices: x_dev[r], y_dev[r] = slab of rank r in the memory of
 * devices[r].  Stream-ordered on every device (lsfc_plan_synchronize waits for all of them).  mode: 0 apply,
 * 1 convolve, 2 convolve with nu. */
int lsfc_multi_apply_dev(lsfc_plan* plan, const double* const* x_dev, double* const* y_dev, int mode);

/* Padded line length the hand-written pipeline uses for an axis of n grid points: the smallest of 2^k, 3*2^k, 5*2^k
 * (32 ... 2048) that is >= 2n; 0 if there is none (such axes run through rocFFT on the exact 2n grid).  Pure host
 * arithmetic, no device needed.  (The reference pads every axis to 4n, src/FastConvolution3D.jl:48.) */
int lsfc_padded_length(int64_t n);

/* ---- errors ---------------------------------------------------------------- */
const char* lsfc_last_error(void);
const char* lsfc_version(void);

#ifdef __cplusplus
}
#endif
#endif /* LSFC_H */
