// Running a plan on device vectors: the passes, the stages of an apply, the batch drivers, the probes that convolve, and the
// apply / timing / profile entry points of the C ABI (gfx950).  Host vectors: host_apply.hip.
#include "plan.hpp"
#include "apply.hpp"
#include "pointwise.hpp"
#include "krylov_blas.hpp"
#include <cmath>
#include <cstring>
#include <functional>
#include <string>

namespace lsfc {

// ---------------------------------------------------------------------------
// the passes (apply.hpp)
// ---------------------------------------------------------------------------
static Slab whole_grid(const lsfc_plan* p) { return Slab{0, p->dims[2]}; }
// the members' vectors at the first plane of a slab
static VecBatch slab_vectors(const lsfc_plan* p, const VecBatch& vb, int nrhs, Slab s) {
    const int64_t off = (int64_t)s.z0 * p->dims[0] * p->dims[1];
    VecBatch v = vb;
    for (int j = 0; j < nrhs; ++j) { v.x[j] += off; v.y[j] += off; }
    return v;
}
static cplx* slab_a1(const lsfc_plan* p, Slab s) { return p->A1.p + (int64_t)s.z0 * p->dims[1] * p->pitch1; }
static cplx* slab_a2(const lsfc_plan* p, Slab s) { return p->A2.p + (int64_t)8 * s.z0; }

// nu (both planes; im null for real nu) at the first plane of a slab, if the pass on side `side` of the convolution is the one
// that multiplies by it
static NuPlanes slab_nu(const lsfc_plan* p, const ConvOp& op, NuSide side, Slab s) {
    if (op.nu != side) return NuPlanes{nullptr, nullptr};
    const int64_t off = (int64_t)s.z0 * p->dims[0] * p->dims[1];
    return NuPlanes{p->nu.p + off, p->nu_im.p ? p->nu_im.p + off : nullptr};
}
// What the passes take (pruned.hpp), for the launches below and for describe_passes alike.
// The x pass on side `side` of the convolution: A1 in rows [line][pitch1 >= Lx], or in the 2D tiles [Lx/8][tile2d] as chunks of width 8
static XPass xpass_args(const lsfc_plan* p, const VecBatch& vb, int nrhs, const ConvOp& op, NuSide side, Slab s) {
    const int Lx = p->pads[0];
    const bool tiles = p->tile2d != 0;
    return XPass{.L = Lx, .vb = slab_vectors(p, vb, nrhs, s), .nrhs = nrhs, .work = slab_a1(p, s), .wbatch = p->a1_elems, .tw = p->tw[0].p,
                 .nlines = (int64_t)p->dims[1] * s.nz, .W = tiles ? 8 : Lx, .Wp = tiles ? 8 : p->pitch1, .n = p->dims[0], .bstride = p->tile2d,
                 .nu = slab_nu(p, op, side, s), .conj = op.conj, .alpha = op.alpha, .beta = op.beta};
}
static YPass ypass_args(const lsfc_plan* p, int nrhs, Slab s) {
    return YPass{.L = p->pads[1], .a1 = slab_a1(p, s), .a2 = slab_a2(p, s), .tw = p->tw[1].p, .Lx = p->pads[0], .m = p->dims[1], .l = s.nz,
                 .p1 = p->pitch1, .p2 = p->pitch2, .nrhs = nrhs, .batch1 = p->a1_elems, .batch2 = p->a2_elems};
}
void pass_xfwd(lsfc_plan* p, const VecBatch& vb, int nrhs, const ConvOp& op, Slab s, hipStream_t st) {
    pruned_xfwd(p->tuning, xpass_args(p, vb, nrhs, op, NuSide::INPUT, s), st);
}
void pass_yfwd(lsfc_plan* p, int nrhs, Slab s, hipStream_t st) { pruned_yfwd(p->tuning, ypass_args(p, nrhs, s), st); }
void pass_yinv(lsfc_plan* p, int nrhs, Slab s, hipStream_t st) { pruned_yinv(p->tuning, ypass_args(p, nrhs, s), st); }
void pass_xinv(lsfc_plan* p, const VecBatch& vb, int nrhs, const ConvOp& op, Slab s, hipStream_t st) {
    pruned_xinv(p->tuning, xpass_args(p, vb, nrhs, op, NuSide::OUTPUT, s), st);
}

// The three geometries of the fused pass.  3D: A2 as tiles [x'/8][Ly][pitch2 >= 8*l] of 8 interleaved z lines, the symbol as
// [x'/8][sym_rows][sym_hz][8]; `Wc` x' storage indices from the tile that `a2_off` / `sym_off` point to (a chunk of a
// distributed plan; the whole range on one device).
static FusedGeom geom_3d(const lsfc_plan* p, int Wc) {
    const int Ly = p->pads[1];
    return FusedGeom{Wc, Ly, (int64_t)p->pitch2 * Ly, (int64_t)p->pitch2, 8, (int64_t)8 * p->sym_hz * p->sym_rows, (int64_t)8 * p->sym_hz, 8,
                     p->ytab.p, p->zmirror.p, p->dims[2]};
}
static FusedPass fused_args_3d(const lsfc_plan* p, int Wc, int64_t a2_off, int64_t sym_off, int nrhs) {
    return FusedPass{.L = p->pads[2], .data = p->A2.p + a2_off, .sym = p->sym.p + sym_off, .tw = p->tw[2].p, .twl = p->twl[2].p, .g = geom_3d(p, Wc),
                     .nrhs = nrhs, .dBatch = p->a2_elems};
}
void plan_zfused_3d(lsfc_plan* p, int Wc, int64_t a2_off, int64_t sym_off, int nrhs, hipStream_t st) {
    pruned_zfused(p->tuning, fused_args_3d(p, Wc, a2_off, sym_off, nrhs), st);
}
// 2D, natural rows: A1 as [m][pitch1 >= Lx], the lines along y; the symbol likewise, [rows][Lx]
static FusedGeom geom_2d_rows(const lsfc_plan* p) {
    return FusedGeom{p->pads[0], 1, 8, 0, (int64_t)p->pitch1, 8, 0, (int64_t)p->pads[0], nullptr, p->zmirror.p, p->dims[1]};
}
// 2D, tiles: A1 as [Lx/8][tile2d >= 8*m] -- the 3D layout with one row per tile; the symbol as [Lx/8][sym_hz][8]
static FusedGeom geom_2d_tiles(const lsfc_plan* p) {
    return FusedGeom{p->pads[0], 1, p->tile2d, 0, 8, (int64_t)8 * p->sym_hz, 0, 8, nullptr, p->zmirror.p, p->dims[1]};
}
// the fused pass of the whole grid: along z on A2 in 3D, along y on A1 in 2D
static FusedPass fused_args(const lsfc_plan* p, int nrhs) {
    if (p->ndim == 3) return fused_args_3d(p, p->pads[0], 0, 0, nrhs);
    return FusedPass{.L = p->pads[1], .data = p->A1.p, .sym = p->sym.p, .tw = p->tw[1].p, .twl = p->twl[1].p,
                     .g = p->tile2d ? geom_2d_tiles(p) : geom_2d_rows(p), .nrhs = nrhs, .dBatch = p->a1_elems};
}
// whether a batch of nrhs right-hand sides shares one launch per pass (lsfc_apply_batch)
static bool batch_fused(const lsfc_plan* p, int nrhs) {
    const bool fuse = p->tuning.batch_fuse > 0 ||
                      (p->tuning.batch_fuse < 0 && (int64_t)p->pads[0] * p->pads[1] * p->pads[2] <= ((int64_t)1 << 24));
    return !(nrhs == 1 || p->dist || p->multi || p->pipeline != lsfc_plan::PRUNED || !fuse);
}
// The kernels an apply of nrhs right-hand sides launches, one line per pass (lsfc_plan_describe_passes): the PassForm of each
// pass from the very arguments pass_xfwd ... pass_xinv hand to the launchers
static std::string describe_passes(const lsfc_plan* p, int nrhs) {
    std::string out = std::string("pipeline=") + lsfc_plan_pipeline(p);
    if (p->multi) return out + " multi-device\n";
    if (p->dist) return out + " distributed\n";
    out += "\n";
    if (p->pipeline != lsfc_plan::PRUNED) return out;
    const bool fused = batch_fused(p, nrhs);
    const int per_launch = fused ? nrhs : 1;
    char line[512];
    auto add = [&](const PassForm& f) { pass_form_print(f, line, sizeof line); out += line; out += "\n"; };
    const bool d3 = p->ndim == 3;
    const Slab all = whole_grid(p);
    const ConvOp op = plan_operator(p);
    add(pruned_xfwd_form(p->tuning, xpass_args(p, VecBatch{}, per_launch, op, NuSide::INPUT, all)));
    if (d3) add(pruned_yfwd_form(p->tuning, ypass_args(p, per_launch, all)));
    add(pruned_zfused_form(p->tuning, fused_args(p, per_launch)));
    if (d3) add(pruned_yinv_form(p->tuning, ypass_args(p, per_launch, all)));
    add(pruned_xinv_form(p->tuning, xpass_args(p, VecBatch{}, per_launch, op, NuSide::OUTPUT, all)));
    // storage: ytab = 1 the y-even half of the symbol rows (each stored row serves a row and its mirror), zmirror = 1 the even half
    // of every symbol line along the fused pass's axis; batch: how nrhs > 1 right-hand sides run through the passes
    snprintf(line, sizeof line, "pitch1=%d pitch2=%d sym_rows=%d sym_hz=%d ytab=%d zmirror=%d tile2d=%lld batch=%s\n", p->pitch1, p->pitch2, p->sym_rows,
             p->sym_hz, (int)(d3 && p->sym_rows != p->pads[1]), (int)(p->zmirror.p != nullptr), (long long)p->tile2d,
             nrhs == 1 ? "none" : (fused ? "fused" : "per_member"));
    out += line;
    return out;
}
void pass_fused(lsfc_plan* p, int nrhs, hipStream_t st) { pruned_zfused(p->tuning, fused_args(p, nrhs), st); }

// ---------------------------------------------------------------------------
// the stages of an apply
// ---------------------------------------------------------------------------
// The single-device apply, stage by stage, in order: visit(name, algorithmic bytes of one right-hand side, run), where run(stream)
// enqueues the stage.  The pruned pipeline takes nrhs <= batch_cap right-hand sides, the rocFFT pipelines one.  The apply and
// the per-stage profile are both visitors of this list, so a pass added here is run and timed alike.  (A template: the apply's
// visitor inlines to the bare calls -- at 48^3 an apply is 36 us of launches, bounded by the host's enqueue time.)
template <class Visit> static void for_each_stage(lsfc_plan* p, int nrhs, const VecBatch& vb, const ConvOp& op, Visit&& visit) {
    // nu_in / nu_out: the 8 B per point of a real nu, the 16 B (two planes) of a complex one, in the pass that multiplies by it
    const double N = (double)p->N, C = 16.0, nu_bytes = p->nu_im.p ? 16 * N : 8 * N;
    const double nu_in = op.nu == NuSide::INPUT ? nu_bytes : 0.0, nu_out = op.nu == NuSide::OUTPUT ? nu_bytes : 0.0;
    if (p->pipeline == lsfc_plan::PRUNED) {
        // (round 3, measured slower and removed again -- profiles/r03_experiment_a1_window.log: the x and y passes chunk by chunk over
        // groups of z planes through one chunk-sized window of A1, hoping the Infinity Cache would absorb the 2 x 4.3 GB of A1 traffic)
        const Slab all = whole_grid(p);
        const bool d3 = p->ndim == 3;
        visit("xfwd", N * C + nu_in + 2 * N * C, [&](hipStream_t st) { pass_xfwd(p, vb, nrhs, op, all, st); });
        if (d3) visit("yfwd", (2 + 4) * N * C, [&](hipStream_t st) { pass_yfwd(p, nrhs, all, st); });
        visit(d3 ? "zfused" : "yfused", d3 ? (4 + 8 + 4) * N * C : (2 + 4 + 2) * N * C, [&](hipStream_t st) { pass_fused(p, nrhs, st); });
        if (d3) visit("yinv", (4 + 2) * N * C, [&](hipStream_t st) { pass_yinv(p, nrhs, all, st); });
        visit("xinv", (2 + 1 + 1) * N * C + nu_out, [&](hipStream_t st) { pass_xinv(p, vb, nrhs, op, all, st); });
    } else {
        const int64_t total = (int64_t)p->pads[0] * p->pads[1] * p->pads[2];
        const double P = (double)total;
        const cplx* x = vb.x[0]; cplx* y = vb.y[0];
        const Slab all = whole_grid(p);
        const NuPlanes nui = slab_nu(p, op, NuSide::INPUT, all), nuo = slab_nu(p, op, NuSide::OUTPUT, all);
        visit("embed", N * C + nu_in + P * C, [&](hipStream_t st) { pw_embed(x, nui.re, p->W.p, p->dims, p->pads, st, op.conj, nui.im); });
        visit("rocfft_fwd", 2 * P * C, [&](hipStream_t st) { p->fwd->exec(p->W.p, st); });
        visit("symbol_mul", 3 * P * C, [&](hipStream_t st) { pw_mul_inplace(p->W.p, p->sym.p, total, st); });
        visit("rocfft_inv", 2 * P * C, [&](hipStream_t st) { p->inv->exec(p->W.p, st); });
        visit("crop_axpy", 3 * N * C + nu_out, [&](hipStream_t st) { pw_crop_axpy(p->W.p, x, y, op.alpha, op.beta, p->dims, p->pads, p->crop, st, nuo.re, op.conj, nuo.im); });
    }
}

// every stage, on the plan's stream
static void run_stages(lsfc_plan* p, int nrhs, const VecBatch& vb, const ConvOp& op) {
    hipStream_t st = p->stream;
    for_each_stage(p, nrhs, vb, op, [st](const char*, double, auto&& run) { run(st); });
}

void plan_convolve_dev(lsfc_plan* p, const cplx* x, cplx* y, const ConvOp& op) {
    if (p->dist) { dist_convolve_dev(p, x, y, op); return; }
    VecBatch vb{}; vb.x[0] = x; vb.y[0] = y;
    run_stages(p, 1, vb, op);
}

void plan_convolve_batch_dev(lsfc_plan* p, int nrhs, const VecBatch& vb, const ConvOp& op) {
    LSFC_REQUIRE(nrhs >= 1 && nrhs <= LSFC_MAX_BATCH, "batch of %d right-hand sides (1..%d per pass)", nrhs, LSFC_MAX_BATCH);
    if (!batch_fused(p, nrhs)) {
        for (int j = 0; j < nrhs; ++j) plan_convolve_dev(p, vb.x[j], vb.y[j], op);
        return;
    }
    if (nrhs > p->batch_cap) {
        // the work arrays hold the batch back to back: grow them (the plan is idle once its stream has drained)
        LSFC_HIP(hipStreamSynchronize(p->stream));
        p->A1.alloc((size_t)(p->a1_elems * nrhs));
        if (p->ndim == 3) p->A2.alloc((size_t)(p->a2_elems * nrhs));
        p->batch_cap = nrhs;
    }
    run_stages(p, nrhs, vb, op);           // (batch_fused: the pruned pipeline)
}

void plan_apply_batch_dev(lsfc_plan* p, const cplx* const* in, cplx* const* out, size_t cnt) {
    for_each_group((int64_t)cnt, in, out, [&](int64_t, int n, const VecBatch& vb) { plan_convolve_batch_dev(p, n, vb, plan_operator(p)); });
}

static void convolve_any(lsfc_plan* p, const double* x, double* y, int64_t nrhs, const ConvOp& op, int memspace) {
    LSFC_REQUIRE(p && x && y, "NULL argument");
    LSFC_REQUIRE(nrhs >= 1, "nrhs must be >= 1");
    if (p->multi) {
        LSFC_REQUIRE(memspace == LSFC_MEM_HOST, "a multi-device plan takes host vectors here; per-device slabs go through lsfc_multi_apply_dev");
    } else {
        LSFC_HIP(hipSetDevice(p->device));
        if (memspace == LSFC_MEM_DEVICE) {
            for_each_group(nrhs, (const cplx*)x, (cplx*)y, p->N, [&](int64_t, int cnt, const VecBatch& vb) { plan_convolve_batch_dev(p, cnt, vb, op); });
            return;
        }
        LSFC_REQUIRE(memspace == LSFC_MEM_HOST, "unknown memspace %d", memspace);
    }
    host_convolve(p, (const cplx*)x, (cplx*)y, nrhs, op);
}

// ---------------------------------------------------------------------------
// probes that convolve
// ---------------------------------------------------------------------------
// kernel samples: the response to a unit source at grid index 0 (one FFT convolution, no nu), built once per plan
void plan_kernel0(lsfc_plan* p) {
    const int64_t N = p->N;
    if (p->kernel0.n == (size_t)N) return;
    p->kernel0.alloc((size_t)N);
    DevBuf<cplx> e; e.alloc((size_t)N);
    LSFC_HIP(hipMemsetAsync(e.p, 0, (size_t)N * sizeof(cplx), p->stream));
    const cplx one = make_double2(1.0, 0.0);
    LSFC_HIP(hipMemcpyAsync(e.p, &one, sizeof one, hipMemcpyHostToDevice, p->stream));
    plan_convolve_dev(p, e.p, p->kernel0.p, conv_plain(false, 0.0, 1.0));
    LSFC_HIP(hipStreamSynchronize(p->stream));
}

// One convolution per further corner of the grid (2^ndim - 1 of them), once per plan.  A kernel that is even along x at
// y >= 0 only is caught by the corner that is last along both, so every corner is visited: first those last along one axis
// (their failure names that axis), then the others (which name their lowest axis).
void plan_require_even_kernel(lsfc_plan* p, const char* who) {
    static const char axis_name[3] = {'x', 'y', 'z'};
    constexpr double TOL = 1e-10;
    if (p->even_dev < 0.0) {
        plan_kernel0(p);
        const int64_t N = p->N;
        DevBuf<cplx> e, r; e.alloc((size_t)N); r.alloc((size_t)N);
        const cplx one = make_double2(1.0, 0.0);
        const int order[7] = {1, 2, 4, 3, 5, 6, 7};
        double worst = 0.0; int axis = 0;
        for (int mask : order) {
            if (mask >> p->ndim) continue;
            int64_t corner = 0, stride = 1;
            for (int a = 0; a < p->ndim; ++a) { if (mask >> a & 1) corner += stride * (p->dims[a] - 1); stride *= p->dims[a]; }
            LSFC_HIP(hipMemsetAsync(e.p, 0, (size_t)N * sizeof(cplx), p->stream));
            LSFC_HIP(hipMemcpyAsync(e.p + corner, &one, sizeof one, hipMemcpyHostToDevice, p->stream));
            plan_convolve_dev(p, e.p, r.p, conv_plain(false, 0.0, 1.0));
            const double d = pw_corner_deviation(r.p, p->kernel0.p, p->dims, mask, p->stream);
            if (d > TOL && !(worst > TOL)) { axis = 0; while (!(mask >> axis & 1)) ++axis; }     // the first corner that fails
            worst = std::max(worst, d);
        }
        p->even_dev = worst; p->even_axis = axis;
    }
    if (p->even_dev > TOL)
        fail(LSFC_EINVAL, "%s: the kernel of this plan is not even along axis %c (deviation %.3e of its largest entry > 1e-10): the rows of its "
                          "Green's matrix are not K[|i - j|], which this entry gathers; the builders' kernels are even, a literal symbol "
                          "(lsfc_plan_create_2d/3d) has to be even in every axis", who, axis_name[p->even_axis], p->even_dev);
}

// The symmetry defect of G as this plan convolves with it (lsfc.h), measured once per plan: two bare convolutions of the probe
// vectors and four reductions on the fixed-order tree.  NaN (an unpatched singular symbol) is kept as NaN and never passes.
static double symmetry_defect(lsfc_plan* p) {
    if (p->sym_defect >= 0.0 || p->sym_defect != p->sym_defect) return p->sym_defect;
    LSFC_HIP(hipSetDevice(p->device));
    const int64_t N = p->N;
    hipStream_t st = p->stream;
    DevBuf<cplx> x, xbar, y, ybar, gx, gy, partial, out;
    for (DevBuf<cplx>* b : { &x, &xbar, &y, &ybar, &gx, &gy }) b->alloc((size_t)N);
    partial.alloc((size_t)blas_partial_count()); out.alloc(4);
    pw_probe(x.p, xbar.p, N, 0, st);
    pw_probe(y.p, ybar.p, N, 1, st);
    const ConvOp bare = conv_plain(false, 0.0, 1.0);
    plan_convolve_dev(p, x.p, gx.p, bare);
    plan_convolve_dev(p, y.p, gy.p, bare);
    blas_dot(ybar.p, gx.p, partial.p, out.p + 0, N, st);          // sum y .* (G x): blas_dot conjugates its first argument
    blas_dot(xbar.p, gy.p, partial.p, out.p + 1, N, st);          // sum x .* (G y)
    blas_nrm2(gx.p, partial.p, out.p + 2, N, st);
    blas_nrm2(y.p, partial.p, out.p + 3, N, st);
    cplx h[4];
    LSFC_HIP(hipMemcpyAsync(h, out.p, sizeof h, hipMemcpyDeviceToHost, st));
    LSFC_HIP(hipStreamSynchronize(st));
    const double den = h[2].x * h[3].x;
    const double num = hypot(h[0].x - h[1].x, h[0].y - h[1].y);
    p->sym_defect = den > 0.0 ? num / den : (num == 0.0 ? 0.0 : NAN);
    return p->sym_defect;
}
// (distributed and multi-device plans know M and the bare convolutions only)
static void require_single_device(const lsfc_plan* plan) {
    LSFC_REQUIRE(!plan->multi, "the transposed and the adjoint operator are not available on a multi-device plan");
    LSFC_REQUIRE(!plan->dist, "the transposed and the adjoint operator are not available on a distributed (or simulated-rank) plan");
}
} // namespace lsfc

using namespace lsfc;

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" {

int lsfc_plan_describe_passes(const lsfc_plan* plan, int nrhs, char* buf, int64_t capacity, int64_t* need) {
    return guarded([&] {
        LSFC_REQUIRE(plan && need, "NULL argument");
        LSFC_REQUIRE(nrhs >= 1 && nrhs <= LSFC_MAX_BATCH, "nrhs must be 1..%d (the right-hand sides of one group of lsfc_apply_batch)", LSFC_MAX_BATCH);
        const std::string text = describe_passes(plan, nrhs);
        *need = (int64_t)text.size() + 1;
        if (buf) {
            LSFC_REQUIRE(capacity >= *need, "buffer too small");
            memcpy(buf, text.c_str(), text.size() + 1);
        }
    });
}

int lsfc_apply(lsfc_plan* plan, const double* x, double* y, int memspace) {
    return guarded([&] { LSFC_REQUIRE(plan, "NULL plan"); convolve_any(plan, x, y, 1, plan_operator(plan), memspace); });
}
int lsfc_convolve(lsfc_plan* plan, const double* x, double* y, int apply_nu, int memspace) {
    return guarded([&] { convolve_any(plan, x, y, 1, conv_plain(apply_nu != 0, 0.0, 1.0), memspace); });
}
int lsfc_apply_batch(lsfc_plan* plan, const double* x, double* y, int64_t nrhs, int mode, int memspace) {
    return guarded([&] {
        LSFC_REQUIRE(plan, "NULL plan");
        LSFC_REQUIRE(mode >= 0 && mode <= 2, "mode must be 0 (apply), 1 (convolve) or 2 (convolve with nu)");
        if (mode == 0) convolve_any(plan, x, y, nrhs, plan_operator(plan), memspace);
        else convolve_any(plan, x, y, nrhs, conv_plain(mode == 2, 0.0, 1.0), memspace);
    });
}

int lsfc_plan_set_op(lsfc_plan* plan, int op) {
    return guarded([&] {
        LSFC_REQUIRE(op == LSFC_OP_N || op == LSFC_OP_T || op == LSFC_OP_H, "op must be LSFC_OP_N, LSFC_OP_T or LSFC_OP_H (got %d)", op);
        LSFC_REQUIRE(plan, "NULL plan");
        if (op != LSFC_OP_N) {
            require_single_device(plan);
            const double d = symmetry_defect(plan);
            // (the op stays what it was: N, since nothing but N gets past this line on such a plan)
            if (!(d <= 1e-10)) fail(LSFC_EINVAL, "the Green's matrix of this plan is not symmetric (symmetry defect %.3e > 1e-10): "
                                                 "I + w^2 diag(nu) G is not its transpose", d);
        }
        plan->op = op;
    });
}
int lsfc_plan_get_op(const lsfc_plan* plan, int* op) {
    return guarded([&] { LSFC_REQUIRE(plan && op, "NULL argument"); *op = plan->op; });
}
int lsfc_plan_symmetry_defect(lsfc_plan* plan, double* defect) {
    return guarded([&] {
        LSFC_REQUIRE(plan && defect, "NULL argument");
        require_single_device(plan);
        *defect = symmetry_defect(plan);
    });
}

int lsfc_sample_sources(lsfc_plan* plan, const int64_t* sources, int64_t nsrc, double* out, int memspace) {
    return guarded([&] {
        LSFC_REQUIRE(plan && sources && out && nsrc >= 1, "bad argument");
        LSFC_REQUIRE(!plan->dist && !plan->multi, "not available on a distributed plan");
        LSFC_HIP(hipSetDevice(plan->device));
        lsfc_plan* p = plan;
        const int64_t N = p->N;
        for (int64_t s = 0; s < nsrc; ++s) LSFC_REQUIRE(sources[s] >= 0 && sources[s] < N, "source index %lld out of range", (long long)sources[s]);
        plan_kernel0(p);
        plan_require_even_kernel(p, "lsfc_sample_sources");
        DevBuf<int64_t> dsrc; dsrc.alloc((size_t)nsrc);
        LSFC_HIP(hipMemcpyAsync(dsrc.p, sources, (size_t)nsrc * sizeof(int64_t), hipMemcpyHostToDevice, p->stream));
        if (memspace == LSFC_MEM_DEVICE) {
            pw_gather_sources(p->kernel0.p, (cplx*)out, dsrc.p, (int)nsrc, p->dims, p->stream);
            LSFC_HIP(hipStreamSynchronize(p->stream));
        } else {
            // stage in batches of at most ~256 MiB
            const int64_t per = std::max<int64_t>(1, ((int64_t)1 << 24) / N);
            DevBuf<cplx> buf; buf.alloc((size_t)(std::min(per, nsrc) * N));
            for (int64_t s0 = 0; s0 < nsrc; s0 += per) {
                const int64_t cnt = std::min(per, nsrc - s0);
                pw_gather_sources(p->kernel0.p, buf.p, dsrc.p + s0, (int)cnt, p->dims, p->stream);
                LSFC_HIP(hipMemcpyAsync((cplx*)out + s0 * N, buf.p, (size_t)(cnt * N) * sizeof(cplx), hipMemcpyDeviceToHost, p->stream));
                LSFC_HIP(hipStreamSynchronize(p->stream));
            }
        }
    });
}

int lsfc_time_apply(lsfc_plan* plan, const double* x_dev, double* y_dev, int reps, double* ms_total) {
    return guarded([&] {
        LSFC_REQUIRE(plan && x_dev && y_dev && ms_total && reps >= 1, "bad argument");
        LSFC_REQUIRE(!plan->multi, "time a multi-device plan from the host around lsfc_multi_apply_dev + lsfc_plan_synchronize");
        LSFC_HIP(hipSetDevice(plan->device));
        hipEvent_t e0, e1;
        LSFC_HIP(hipEventCreate(&e0)); LSFC_HIP(hipEventCreate(&e1));
        LSFC_HIP(hipEventRecord(e0, plan->stream));
        for (int r = 0; r < reps; ++r) plan_apply_dev(plan, (const cplx*)x_dev, (cplx*)y_dev);
        LSFC_HIP(hipEventRecord(e1, plan->stream));
        LSFC_HIP(hipEventSynchronize(e1));
        float ms = 0; LSFC_HIP(hipEventElapsedTime(&ms, e0, e1));
        *ms_total = ms;
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    });
}

int lsfc_profile_apply(lsfc_plan* plan, const double* x_dev, double* y_dev, int reps, int max_stages, const char** names,
                       double* ms, double* bytes, int* nstages) {
    return guarded([&] {
        LSFC_REQUIRE(plan && names && ms && bytes && nstages && reps >= 1, "bad argument");
        if (plan->multi) { multi_profile(plan, reps, max_stages, names, ms, bytes, nstages); return; }    // (on the ranks' staging vectors)
        LSFC_REQUIRE(x_dev && y_dev, "bad argument");
        LSFC_HIP(hipSetDevice(plan->device));
        lsfc_plan* p = plan;
        hipStream_t st = p->stream;
        VecBatch vb{}; vb.x[0] = (const cplx*)x_dev; vb.y[0] = (cplx*)y_dev;
        const ConvOp op = plan_operator(p);            // the operator lsfc_plan_set_op selected
        // the stages of the apply (for_each_stage), or those a distributed plan lists
        struct Stage { const char* name; double bytes; std::function<void()> run; };
        std::vector<Stage> dstages;
        if (p->dist) dist_profile_stages(p, vb.x[0], vb.y[0], [&](const char* name, double b, std::function<void()> run) { dstages.push_back({name, b, std::move(run)}); });
        auto walk = [&](auto&& visit) {
            if (p->dist) for (Stage& s : dstages) visit(s.name, s.bytes, [&s](hipStream_t) { s.run(); });
            else for_each_stage(p, 1, vb, op, visit);
        };
        int ns = 0;
        walk([&](const char* name, double b, auto&&) { if (ns < max_stages) { names[ns] = name; bytes[ns] = b; ms[ns] = 0.0; } ++ns; });
        LSFC_REQUIRE(ns <= max_stages, "max_stages too small (need %d)", ns);
        *nstages = ns;
        std::vector<hipEvent_t> ev((size_t)ns + 1);
        for (auto& e : ev) LSFC_HIP(hipEventCreate(&e));
        for (int r = 0; r < reps; ++r) {
            // an event after every stage
            int i = 0;
            LSFC_HIP(hipEventRecord(ev[0], st));
            walk([&](const char*, double, auto&& run) { run(st); ++i; LSFC_HIP(hipEventRecord(ev[(size_t)i], st)); });
            LSFC_HIP(hipEventSynchronize(ev[(size_t)ns]));
            for (int k = 0; k < ns; ++k) { float t = 0; LSFC_HIP(hipEventElapsedTime(&t, ev[(size_t)k], ev[(size_t)k + 1])); ms[k] += t; }
        }
        for (int k = 0; k < ns; ++k) ms[k] /= reps;
        for (auto& e : ev) (void)hipEventDestroy(e);
    });
}

} // extern "C"
