// lsfc C ABI: what makes and owns a plan -- the error buffer, the rocFFT wrapper, the three ways a symbol becomes a plan, the
// plan's settings, the memory helpers (gfx950).  Running a plan: apply.hip, host_apply.hip.
#include "plan.hpp"
#include "pointwise.hpp"
#include <cmath>
#include <cstring>
#include <mutex>

namespace lsfc {

// ---------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------
static thread_local char g_last_error[1024] = "";
void set_last_error(const char* fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(g_last_error, sizeof g_last_error, fmt, ap); va_end(ap);
}

// ---------------------------------------------------------------------------
// rocFFT wrapper
// ---------------------------------------------------------------------------
#define LSFC_ROCFFT(expr) do { rocfft_status s_ = (expr); if (s_ != rocfft_status_success) \
    ::lsfc::fail(LSFC_EHIP, "%s failed with rocfft_status %d (%s:%d)", #expr, (int)s_, __FILE__, __LINE__); } while (0)

void rocfft_global_setup() {
    static std::once_flag once;
    std::call_once(once, [] { rocfft_setup(); });
}

RocFft::~RocFft() { release(); }
void RocFft::release() {
    if (info) { rocfft_execution_info_destroy(info); info = nullptr; }
    if (plan) { rocfft_plan_destroy(plan); plan = nullptr; }
    work.release();
}
void RocFft::finish_create() {
    size_t wsz = 0;
    LSFC_ROCFFT(rocfft_plan_get_work_buffer_size(plan, &wsz));
    LSFC_ROCFFT(rocfft_execution_info_create(&info));
    if (wsz) { work.alloc(wsz); LSFC_ROCFFT(rocfft_execution_info_set_work_buffer(info, work.p, wsz)); }
}
void RocFft::create(int ndim, const size_t* lengths, bool forward, size_t batch, bool lazy_work) {
    rocfft_global_setup();
    // drop unit dimensions
    size_t len[3]; int nd = 0;
    for (int d = 0; d < ndim; ++d) if (lengths[d] > 1) len[nd++] = lengths[d];
    if (nd == 0) { len[0] = 1; nd = 1; }
    LSFC_ROCFFT(rocfft_plan_create(&plan, rocfft_placement_inplace,
                                   forward ? rocfft_transform_type_complex_forward : rocfft_transform_type_complex_inverse,
                                   rocfft_precision_double, nd, len, batch, nullptr));
    if (!lazy_work) finish_create();
}
void RocFft::create_strided_1d(size_t length, size_t stride, size_t dist, size_t batch, bool forward, bool lazy_work) {
    rocfft_global_setup();
    rocfft_plan_description desc = nullptr;
    LSFC_ROCFFT(rocfft_plan_description_create(&desc));
    const size_t strides[1] = { stride };
    rocfft_status s = rocfft_plan_description_set_data_layout(desc, rocfft_array_type_complex_interleaved, rocfft_array_type_complex_interleaved,
                                                              nullptr, nullptr, 1, strides, dist, 1, strides, dist);
    if (s == rocfft_status_success)
        s = rocfft_plan_create(&plan, rocfft_placement_inplace,
                               forward ? rocfft_transform_type_complex_forward : rocfft_transform_type_complex_inverse,
                               rocfft_precision_double, 1, &length, batch, desc);
    rocfft_plan_description_destroy(desc);
    LSFC_ROCFFT(s);
    if (!lazy_work) finish_create();
}
void RocFft::exec(void* buf, hipStream_t stream) {
    if (!info) finish_create();
    LSFC_ROCFFT(rocfft_execution_info_set_stream(info, stream));
    void* in[1] = { buf };
    LSFC_ROCFFT(rocfft_execute(plan, in, nullptr, info));
}

// ---------------------------------------------------------------------------
// plan construction helpers
// ---------------------------------------------------------------------------
// (environment switches, developer knobs, read at plan creation)
// LSFC_SYM_EVEN_Y=0 / LSFC_SYM_EVEN_Z=0: store the full symbol although it is even in y / along the fused pass's axis
static bool sym_even_y_enabled() { return env_switch("LSFC_SYM_EVEN_Y") != '0'; }
static bool sym_even_z_enabled() { return env_switch("LSFC_SYM_EVEN_Z") != '0'; }

void select_device(int device, const char* what, bool say_why) {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        const char* why = e == hipSuccess ? "device count is 0" : hipGetErrorString(e);
        if (say_why) fail(LSFC_ENODEV, "no HIP device available (%s): the %s has no CPU fallback", why, what);
        fail(LSFC_ENODEV, "no HIP device available: the %s has no CPU fallback", what);
    }
    LSFC_REQUIRE(device >= 0 && device < count, "device %d out of range (have %d)", device, count);
    LSFC_HIP(hipSetDevice(device));
}

void plan_common_init(lsfc_plan* p, int ndim, int64_t n, int64_t m, int64_t l, const double* nu_host, double omega,
                      int quad_rule, unsigned flags, int device) {
    LSFC_REQUIRE(n >= 1 && m >= 1 && l >= 1 && n <= 8192 && m <= 8192 && l <= 8192, "grid size out of range");
    LSFC_REQUIRE(quad_rule == LSFC_QUAD_TRAPEZOIDAL || quad_rule == LSFC_QUAD_GREENGARD_VICO,
                 "unknown quadRule %d (the reference leaves B undefined, src/FastConvolution.jl:106)", quad_rule);
    LSFC_REQUIRE(nu_host != nullptr, "nu is NULL");
    select_device(device, "lsfc operator", true);
    pruned_warmup(device);
    p->device = device; p->ndim = ndim;
    p->dims[0] = (int)n; p->dims[1] = (int)m; p->dims[2] = (int)l;
    p->N = n * m * l; p->omega = omega; p->quad_rule = quad_rule; p->flags = flags;
    p->nu.alloc((size_t)p->N);
    LSFC_HIP(hipMemcpy(p->nu.p, nu_host, p->N * sizeof(double), hipMemcpyHostToDevice));
    p->tuning = pruned_default_tuning();
}

void plan_make_twiddles(lsfc_plan* p, int axis, int L) {
    std::vector<cplx> tw((size_t)L);
    for (int j = 0; j < L; ++j) {
        const long double a = -2.0L * 3.14159265358979323846264338327950288L * (long double)j / (long double)L;
        tw[j] = make_double2((double)cosl(a), (double)sinl(a));
    }
    p->tw[axis].alloc((size_t)L);
    LSFC_HIP(hipMemcpy(p->tw[axis].p, tw.data(), (size_t)L * sizeof(cplx), hipMemcpyHostToDevice));
    std::vector<cplx> full((size_t)pruned_twfull_len(L) + 1);
    pruned_twfull(L, tw.data(), full.data());
    p->twl[axis].alloc(full.size());
    LSFC_HIP(hipMemcpy(p->twl[axis].p, full.data(), full.size() * sizeof(cplx), hipMemcpyHostToDevice));
}

// The hand-written pipeline works on L = the smallest of 2^k, 3*2^k, 5*2^k that is >= 2n, per axis (the grid itself
// may have any size: lines are zero-extended in registers).  It is chosen unless that embedding would more than
// quadruple the number of grid points (tiny or very elongated grids), where the monolithic rocFFT transform on the
// exact 2n grid is the better deal.
static bool pruned_eligible(const lsfc_plan* p) {
    if (p->flags & (LSFC_FLAG_FORCE_ROCFFT | LSFC_FLAG_LITERAL_PAD)) return false;
    double ratio = 1.0;
    for (int d = 0; d < p->ndim; ++d) {
        const int L = pruned_best_length(p->dims[d]);
        if (L == 0) return false;
        // the slab-wise Greengard-Vico generator samples the literal 4n lattice: a working line longer than 4n (an axis of
        // fewer than 8 points next to long ones) has no such samples -> exact 2n grid through rocFFT
        if (p->ndim == 3 && L > 4 * p->dims[d]) return false;
        ratio *= (double)L / (2.0 * (double)p->dims[d]);
    }
    return ratio <= 4.0;
}

// working padded grid of the reduced pipelines: pruned_best_length(n) (pruned) or 2n (rocFFT); sets p->pads / p->pipeline
static void plan_choose_reduced_grid(lsfc_plan* p) {
    const bool pr = pruned_eligible(p);
    for (int d = 0; d < 3; ++d) {
        p->crop[d] = 0;
        if (d >= p->ndim) p->pads[d] = 1;
        else p->pads[d] = pr ? pruned_best_length(p->dims[d]) : 2 * p->dims[d];
    }
    p->pipeline = pr ? lsfc_plan::PRUNED : lsfc_plan::ROCFFT_REDUCED;
}

static void setup_rocfft_pipeline(lsfc_plan* p) {
    const size_t len[3] = { (size_t)p->pads[0], (size_t)p->pads[1], (size_t)p->pads[2] };
    p->fwd.reset(new RocFft()); p->fwd->create(3, len, true);
    p->inv.reset(new RocFft()); p->inv->create(3, len, false);
    p->W.alloc(len[0] * len[1] * len[2]);
}

// Finish a plan from a natural-layout symbol already on the device: Gd has p->pads entries; centred => ifftshift is folded in.
static void plan_finish_literal(lsfc_plan* p, const cplx* Gd, bool centred) {
    // working grid == the caller's padded grid; symbol pre-shifted and pre-scaled once
    const int64_t total = (int64_t)p->pads[0] * p->pads[1] * p->pads[2];
    p->sym.alloc((size_t)total);
    int shift[3];
    for (int d = 0; d < 3; ++d) shift[d] = centred ? p->pads[d] / 2 : 0;
    pw_roll_scale(Gd, p->sym.p, p->pads, shift, 1.0 / (double)total, p->stream);
    p->pipeline = lsfc_plan::ROCFFT_LITERAL;
    setup_rocfft_pipeline(p);
    LSFC_HIP(hipStreamSynchronize(p->stream));
}

// Even symbol along the fused pass's axis: a line of L points stores only the frequencies k <= L/2 -- the storage slots
// s < L/2 plus the k = L/2 entry at index L/2 -- and the kernel fetches the value of every upper slot from its mirror.
// perm[s] = frequency held at storage slot s.  Returns the precondition "slot s < L/2 <=> frequency < L/2" (true for every
// factorisation in fft_configs.hpp); if it holds and zm != NULL, zm[s - L/2] = where the stored line holds frequency
// (L - perm[s]) mod L, for the L/2 upper slots s.
static bool mirror_slots(const std::vector<int>& perm, std::vector<int>* zm) {
    const int L = (int)perm.size();
    for (int s = 0; s < L; ++s) if ((perm[(size_t)s] < L / 2) != (s < L / 2)) return false;
    if (!zm) return true;
    std::vector<int> inv((size_t)L);
    for (int s = 0; s < L; ++s) inv[(size_t)perm[(size_t)s]] = s;
    zm->resize((size_t)L / 2);
    for (int s = L / 2; s < L; ++s) {
        const int km = (L - perm[(size_t)s]) % L;                    // in [1, L/2]
        (*zm)[(size_t)(s - L / 2)] = (km == L / 2) ? L / 2 : inv[(size_t)km];
    }
    return true;
}
static void upload_mirror_slots(lsfc_plan* p, const std::vector<int>& zm) {
    p->zmirror.alloc(zm.size());
    LSFC_HIP(hipMemcpy(p->zmirror.p, zm.data(), zm.size() * sizeof(int), hipMemcpyHostToDevice));
}

void plan_setup_symbol_rows(lsfc_plan* p, const cplx* G2, const std::vector<int>& perm_y, const std::vector<int>& perm_z, DevBuf<int>& pyrow) {
    const int Ly = p->pads[1], Lz = p->pads[2];
    // The Green's symbols of the reference are even in every axis.  When the reduced symbol handed to us is even in
    // y (checked numerically: the literal-symbol constructors accept arbitrary data) only the rows with ky <= Ly/2
    // are stored, and each row is scheduled right next to its mirror: the second read of the shared symbol row is
    // served on-die by the Infinity Cache, which removes ~1/8 of the apply's HBM traffic.
    bool even = false;
    // (G2 == NULL: the caller built the symbol through its symmetry, symbol_gv3d_quarter, and vouches for it)
    if (sym_even_y_enabled() && p->ndim == 3 && Ly >= 4) even = !G2 || pw_mirror_deviation(G2, p->pads, 1, p->stream) < 1e-13;
    std::vector<int> inv((size_t)Ly), rowky;
    for (int s = 0; s < Ly; ++s) inv[perm_y[s]] = s;
    std::vector<int2> tab;
    if (even) {
        std::vector<int> rowof((size_t)Ly, -1);
        for (int s = 0; s < Ly; ++s) if (perm_y[s] <= Ly / 2) { rowof[s] = (int)rowky.size(); rowky.push_back(perm_y[s]); }
        // block order: the self-mirrored rows (ky = 0, Ly/2) first, then every row followed by its mirror -- with an even
        // number of the former every pair sits at (2j, 2j + 1), which the ticketed fused pass relies on to send both rows
        // of a pair through the same L2
        for (int s = 0; s < Ly; ++s)
            if (rowof[s] >= 0 && inv[(Ly - perm_y[s]) % Ly] == s) tab.push_back(make_int2(s, rowof[s]));
        for (int s = 0; s < Ly; ++s) {
            if (rowof[s] < 0) continue;
            const int mirror = inv[(Ly - perm_y[s]) % Ly];
            if (mirror == s) continue;
            tab.push_back(make_int2(s, rowof[s]));
            tab.push_back(make_int2(mirror, rowof[s]));
        }
    } else {
        for (int s = 0; s < Ly; ++s) { rowky.push_back(perm_y[s]); tab.push_back(make_int2(s, s)); }
    }
    LSFC_REQUIRE((int)tab.size() == Ly, "internal: row table has %d entries for %d rows", (int)tab.size(), Ly);
    p->sym_rows = (int)rowky.size();
    p->ytab.alloc(tab.size());
    LSFC_HIP(hipMemcpy(p->ytab.p, tab.data(), tab.size() * sizeof(int2), hipMemcpyHostToDevice));
    pyrow.alloc(rowky.size());
    LSFC_HIP(hipMemcpy(pyrow.p, rowky.data(), rowky.size() * sizeof(int), hipMemcpyHostToDevice));

    // z-even symbol: store only kz <= Lz/2 per line; the kernel fetches the mirror values of its upper slots from
    // the threads that loaded them (through LDS): mirror_slots.
    std::vector<int> zm;
    bool zeven = false;
    if (sym_even_z_enabled() && p->ndim == 3 && Lz >= 32 && mirror_slots(perm_z, &zm))
        zeven = !G2 || pw_mirror_deviation(G2, p->pads, 2, p->stream) < 1e-13;
    if (zeven) {
        p->sym_hz = Lz / 2 + 8;
        upload_mirror_slots(p, zm);
    } else {
        p->sym_hz = Lz;
        p->zmirror.release();
    }
}

// whether the pruned pipeline will store the y-even, z-even quarter of a 3D symbol that is even in every axis
bool plan_quarter_symbol_ok(const lsfc_plan* p) {
    if (p->ndim != 3) return false;                    // (the caller knows that the plan runs the pruned pipeline)
    // (LSFC_SYMBOL_FULL=1: evaluate the symbol on the whole grid although its symmetry would do)
    if (!sym_even_y_enabled() || !sym_even_z_enabled() || env_switch("LSFC_SYMBOL_FULL") == '1') return false;
    const int Ly = p->pads[1], Lz = p->pads[2];
    if (Ly < 4 || Lz < 32 || p->pads[0] % 2 || Ly % 2 || Lz % 2) return false;
    std::vector<int> pz((size_t)Lz);
    pruned_perm(Lz, pz.data());
    return mirror_slots(pz, nullptr);
}

// G2: natural FFT-order symbol on the grid chosen by plan_choose_reduced_grid, unscaled; quarter: only its rows ky <= Ly/2
// and planes kz <= Lz/2 (symbol_gv3d_quarter)
static void plan_finish_symbol(lsfc_plan* p, DevBuf<cplx>& G2, bool quarter) {
    const int64_t total = (int64_t)p->pads[0] * p->pads[1] * p->pads[2];
    const int64_t have = quarter ? (int64_t)p->pads[0] * (p->pads[1] / 2 + 1) * (p->pads[2] / 2 + 1) : total;
    LSFC_REQUIRE((int64_t)G2.n == have, "internal: reduced symbol has %lld entries, expected %lld", (long long)G2.n, (long long)have);
    LSFC_REQUIRE(!quarter || (p->pipeline == lsfc_plan::PRUNED && p->ndim == 3), "internal: quarter symbol outside the 3D pruned pipeline");
    const double scale = 1.0 / (double)total;
    if (p->pipeline == lsfc_plan::PRUNED) {
        std::vector<int> perm[3];
        DevBuf<int> dperm[3], pyrow, zero, drow;        // tables the queued pw_permute_symbol reads: they live until the synchronisation below
        for (int d = 0; d < p->ndim; ++d) {
            perm[d].resize((size_t)p->pads[d]);
            pruned_perm(p->pads[d], perm[d].data());
            dperm[d].alloc(perm[d].size());
            LSFC_HIP(hipMemcpy(dperm[d].p, perm[d].data(), perm[d].size() * sizeof(int), hipMemcpyHostToDevice));
            plan_make_twiddles(p, d, p->pads[d]);
        }
        if (p->ndim == 3) {
            plan_setup_symbol_rows(p, quarter ? nullptr : G2.p, perm[1], perm[2], pyrow);
            LSFC_REQUIRE(!quarter || (p->sym_rows == p->pads[1] / 2 + 1 && p->sym_hz == p->pads[2] / 2 + 8), "internal: quarter symbol but full storage");
            p->sym.alloc((size_t)p->pads[0] * p->sym_rows * p->sym_hz);
            pw_permute_symbol(G2.p, p->sym.p, dperm[0].p, pyrow.p, dperm[2].p, p->pads, p->sym_rows, p->sym_hz, 0, p->pads[0] / 8, scale, p->stream,
                              quarter ? p->pads[1] / 2 + 1 : 0);
        } else {
            // 2D: the fused pass runs along y.  An even symbol (every Green's symbol of the reference) is stored for the
            // frequencies ky <= Ly/2 only -- rows s < Ly/2 in storage order plus the ky = Ly/2 row -- and the fused pass
            // fetches the mirror values through LDS exactly as the 3D pass does along z (half the symbol bytes of the pass).
            const int Ly = p->pads[1];
            std::vector<int> zm;
            bool even = false;
            if (sym_even_z_enabled() && Ly >= 32 && mirror_slots(perm[1], &zm)) even = pw_mirror_deviation(G2.p, p->pads, 1, p->stream) < 1e-13;
            if (even) {
                upload_mirror_slots(p, zm);
                // Tiled form (default from Ly = 2048 on; LSFC_2D_TILED=0|1): the x passes write / read the x'-expanded array as
                // tiles [Lx/8][m][8] -- the chunked output they already have for the slab transposes, chunk width 8 -- so the
                // fused pass along y finds its eight interleaved lines in ONE contiguous run of 128-B lines, exactly the 3D fused
                // pass's situation (same kernels, same z-even symbol layout), instead of 64-B pieces a whole row apart.
                const int t2 = env_switch("LSFC_2D_TILED");
                const bool tiled = t2 >= 0 ? t2 == '1' : Ly >= 2048;    // (at 1024 points the 8-line tiles are too few for the chip: 128 workgroups)
                // (the tiled fused pass is the 3D half-tile kernel: whole groups of 8 tiles -- Lx / 8 tiles here; a short x axis,
                // e.g. n = 80 next to m = 1024, keeps the natural rows)
                if (tiled && p->pads[0] % 8 == 0 && (p->pads[0] / 8) % 8 == 0 && p->pads[0] <= 2048) {
                    p->sym_hz = Ly / 2 + 8; p->sym_rows = 1;
                    zero.alloc(1);
                    LSFC_HIP(hipMemset(zero.p, 0, sizeof(int)));
                    const int L3[3] = { p->pads[0], 1, Ly };        // the line axis plays z; one symbol row per tile
                    p->sym.alloc((size_t)p->pads[0] * p->sym_hz);
                    pw_permute_symbol(G2.p, p->sym.p, dperm[0].p, zero.p, dperm[1].p, L3, 1, p->sym_hz, 0, p->pads[0] / 8, scale, p->stream);
                    p->tile2d = (int64_t)8 * p->dims[1] + (Ly >= 1024 ? 72 : 0);
                } else {
                    std::vector<int> rowk(perm[1].begin(), perm[1].begin() + Ly / 2);     // rows ky < Ly/2 in storage order, then ky = Ly/2
                    rowk.push_back(Ly / 2);
                    drow.alloc(rowk.size());
                    LSFC_HIP(hipMemcpy(drow.p, rowk.data(), rowk.size() * sizeof(int), hipMemcpyHostToDevice));
                    p->sym.alloc((size_t)p->pads[0] * rowk.size());
                    pw_permute_symbol(G2.p, p->sym.p, dperm[0].p, drow.p, dperm[2].p, p->pads, (int)rowk.size(), 1, 0, p->pads[0] / 8, scale, p->stream);
                }
            } else {
                p->zmirror.release();
                p->sym.alloc((size_t)total);
                pw_permute_symbol(G2.p, p->sym.p, dperm[0].p, dperm[1].p, dperm[2].p, p->pads, p->pads[1], 1, 0, p->pads[0] / 8, scale, p->stream);
            }
        }
        LSFC_HIP(hipStreamSynchronize(p->stream));
        G2.release();
        // row padding of the work arrays (auto: at 2m >= 1024 the 16-KB / 64-KB power-of-two row strides of the y passes
        // are broken up by +40 / +72 elements: yfwd 2.86 -> 2.59 ms, yinv 2.92 -> 2.57 ms at 512^3; neutral or worse below)
        const bool big = p->ndim == 3 && p->pads[1] >= 1024;
        const int pad1 = p->tuning.pad1 >= 0 ? p->tuning.pad1 : (big ? 40 : 0);
        const int pad2 = p->tuning.pad2 >= 0 ? p->tuning.pad2 : (big ? 72 : 0);
        p->pitch1 = p->pads[0] + ((p->ndim == 3) ? pad1 / 8 * 8 : 0);
        p->pitch2 = 8 * p->dims[2] + pad2 / 8 * 8;
        p->a1_elems = (int64_t)p->pitch1 * p->dims[1] * p->dims[2];
        if (p->tile2d) p->a1_elems = std::max<int64_t>(p->a1_elems, p->tile2d * (p->pads[0] / 8));
        p->a2_elems = (p->ndim == 3) ? (int64_t)p->pitch2 * p->pads[1] * (p->pads[0] / 8) : 0;
        p->A1.alloc((size_t)p->a1_elems);
        if (p->ndim == 3) p->A2.alloc((size_t)p->a2_elems);
        p->batch_cap = 1;
    } else {
        pw_scale(G2.p, scale, total, p->stream);
        LSFC_HIP(hipStreamSynchronize(p->stream));
        p->sym = std::move(G2);
        setup_rocfft_pipeline(p);
    }
}

// reduce a (pe,me,le) symbol (centred or FFT order) to the working grid and pick the pipeline
static void plan_finish_reduce(lsfc_plan* p, DevBuf<cplx>& Gd, const int lit[3], bool centred, const int kernel_origin[3]) {
    // T = ifft(ifftshift(G)) on the literal grid is the spatial kernel; the cropped convolution only needs its
    // offsets -(n-1)..n-1 per axis, so it is re-sampled on the working grid q and transformed back: G2 = fft(T2).
    //   Greengard-Vico: offset d sits at index d mod lit (kernel_origin = 0), crop window [0, n).
    //   trapezoidal:    offset d sits at index d + (n-1) (kernel_origin = n-1; crop window [n-1, 2n-2] of the reference).
    plan_choose_reduced_grid(p);
    const int* q = p->pads;
    for (int d = 0; d < p->ndim; ++d)
        LSFC_REQUIRE(lit[d] >= 2 * p->dims[d] - 1, "padded size %d along axis %d is smaller than 2n-1=%d", lit[d], d, 2 * p->dims[d] - 1);
    const int64_t ltotal = (int64_t)lit[0] * lit[1] * lit[2];
    const int64_t qtotal = (int64_t)q[0] * q[1] * q[2];
    {
        DevBuf<cplx> tmp; tmp.alloc((size_t)ltotal);
        int shift[3]; for (int d = 0; d < 3; ++d) shift[d] = centred ? lit[d] / 2 : 0;
        pw_roll_scale(Gd.p, tmp.p, lit, shift, 1.0, p->stream);
        LSFC_HIP(hipStreamSynchronize(p->stream));
        Gd.release();
        const size_t len[3] = { (size_t)lit[0], (size_t)lit[1], (size_t)lit[2] };
        RocFft inv; inv.create(3, len, false);
        inv.exec(tmp.p, p->stream);
        Gd.alloc((size_t)qtotal);
        int nmax[3]; for (int d = 0; d < 3; ++d) nmax[d] = (d < p->ndim) ? p->dims[d] - 1 : 0;
        pw_resample_kernel(tmp.p, Gd.p, lit, q, kernel_origin, nmax, 1.0 / (double)ltotal, p->stream);
        LSFC_HIP(hipStreamSynchronize(p->stream));
    }
    {
        const size_t len[3] = { (size_t)q[0], (size_t)q[1], (size_t)q[2] };
        RocFft fwd; fwd.create(3, len, true);
        fwd.exec(Gd.p, p->stream);
        LSFC_HIP(hipStreamSynchronize(p->stream));
    }
    plan_finish_symbol(p, Gd, false);
}

// Finish a plan from a symbol on its literal grid `lit` (on the device; centred or FFT order), the kernel's zero offset at index
// kernel_origin: on that very grid under LSFC_FLAG_LITERAL_PAD -- the crop window starts at the kernel origin --, else reduced
static void plan_finish_from_literal(lsfc_plan* p, DevBuf<cplx>& Gd, const int lit[3], bool centred, const int kernel_origin[3]) {
    if (p->flags & LSFC_FLAG_LITERAL_PAD) {
        for (int d = 0; d < 3; ++d) { p->pads[d] = lit[d]; p->crop[d] = kernel_origin[d]; }
        plan_finish_literal(p, Gd.p, centred);
    } else plan_finish_reduce(p, Gd, lit, centred, kernel_origin);
}

} // namespace lsfc

using namespace lsfc;

lsfc_plan::lsfc_plan() {}
lsfc_plan::~lsfc_plan() {}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" {

const char* lsfc_last_error(void) { return g_last_error; }
int lsfc_padded_length(int64_t n) { return (n >= 1 && n <= 1024) ? lsfc::pruned_best_length(n) : 0; }
int lsfc_storage_order(int64_t L, int64_t* freq_of_slot) {
    return guarded([&] {
        LSFC_REQUIRE(freq_of_slot, "NULL argument");
        LSFC_REQUIRE(L >= 1 && L <= 2048 && pruned_length_supported(L), "the pruned pipeline has no lines of %lld points", (long long)L);
        std::vector<int> perm((size_t)L);
        pruned_perm((int)L, perm.data());
        for (int64_t s = 0; s < L; ++s) freq_of_slot[s] = perm[(size_t)s];
    });
}

const char* lsfc_version(void) { return "lsfc 0.1 (gfx950, rocFFT + hand-written pruned FFT passes)"; }

static int create_from_literal(lsfc_plan** out, int ndim, int64_t n, int64_t m, int64_t l, int64_t ne, int64_t me, int64_t le,
                               const double* nu, const double* gfft, double omega, int quad_rule, unsigned flags, int device) {
    return guarded([&] {
        LSFC_REQUIRE(out && gfft, "NULL argument");
        *out = nullptr;
        std::unique_ptr<lsfc_plan> p(new lsfc_plan());
        plan_common_init(p.get(), ndim, n, m, l, nu, omega, quad_rule, flags, device);
        LSFC_REQUIRE(ne >= 1 && me >= 1 && le >= 1 && ne <= 16384 && me <= 16384 && le <= 16384, "padded size out of range");
        const int lit[3] = { (int)ne, (int)me, (int)le };
        const int64_t ltotal = ne * me * le;
        DevBuf<cplx> Gd; Gd.alloc((size_t)ltotal);
        LSFC_HIP(hipMemcpy(Gd.p, gfft, (size_t)ltotal * sizeof(cplx), hipMemcpyHostToDevice));
        const bool trap = quad_rule == LSFC_QUAD_TRAPEZOIDAL;
        // trapezoidal: plain FFT-order symbol on the (2n-1) grid, crop window [n-1, 2n-2] (src/FastConvolution.jl:70-82)
        for (int d = 0; d < ndim; ++d)
            LSFC_REQUIRE(lit[d] >= (trap ? 2 * p->dims[d] - 1 : p->dims[d]), "padded size %d too small along axis %d", lit[d], d);
        int origin[3]; for (int d = 0; d < 3; ++d) origin[d] = (trap && d < ndim) ? p->dims[d] - 1 : 0;
        plan_finish_from_literal(p.get(), Gd, lit, !trap, origin);
        *out = p.release();
    });
}

int lsfc_plan_create_2d(lsfc_plan** out, int64_t n, int64_t m, int64_t ne, int64_t me, const double* nu, const double* gfft,
                        double omega, int quad_rule, unsigned flags, int device) {
    return create_from_literal(out, 2, n, m, 1, ne, me, 1, nu, gfft, omega, quad_rule, flags, device);
}
int lsfc_plan_create_3d(lsfc_plan** out, int64_t n, int64_t m, int64_t l, int64_t ne, int64_t me, int64_t le, const double* nu,
                        const double* gfft, double omega, int quad_rule, unsigned flags, int device) {
    return create_from_literal(out, 3, n, m, l, ne, me, le, nu, gfft, omega, quad_rule, flags, device);
}

int lsfc_plan_create_gv3d(lsfc_plan** out, int64_t n, int64_t m, int64_t l, double box, double omega, const double* nu,
                          unsigned flags, int device) {
    return guarded([&] {
        LSFC_REQUIRE(out, "NULL argument"); *out = nullptr;
        LSFC_REQUIRE(n % 2 == 0 && m % 2 == 0 && l % 2 == 0, "buildFastConvolution3D: even n only (the reference's odd branch is broken)");
        LSFC_REQUIRE(box > 0, "box must be positive");
        PhaseTimer pt;
        std::unique_ptr<lsfc_plan> p(new lsfc_plan());
        plan_common_init(p.get(), 3, n, m, l, nu, omega, LSFC_QUAD_GREENGARD_VICO, flags & ~LSFC_FLAG_LITERAL_PAD, device);
        pt.mark("init + nu upload");
        DevBuf<cplx> G2;
        plan_choose_reduced_grid(p.get());
        if (p->pipeline == lsfc_plan::PRUNED && plan_quarter_symbol_ok(p.get())) {
            symbol_gv3d_quarter(p.get(), box, G2);
            pt.mark("symbol (total; through its symmetry)");
            plan_finish_symbol(p.get(), G2, true);
        } else {
            symbol_gv3d_reduced(p.get(), box, G2);
            pt.mark("symbol (total)");
            plan_finish_symbol(p.get(), G2, false);
        }
        pt.mark("tables, symbol permutation, work arrays");
        p->even_dev = 0.0;                 // a function of kx^2 + ky^2 + kz^2 (plan_require_even_kernel)
        *out = p.release();
    });
}

int lsfc_plan_create_gv2d(lsfc_plan** out, int64_t n, int64_t m, double box, double omega, const double* nu, unsigned flags, int device) {
    return guarded([&] {
        LSFC_REQUIRE(out, "NULL argument"); *out = nullptr;
        LSFC_REQUIRE(box > 0, "box must be positive");
        std::unique_ptr<lsfc_plan> p(new lsfc_plan());
        plan_common_init(p.get(), 2, n, m, 1, nu, omega, LSFC_QUAD_GREENGARD_VICO, flags, device);
        DevBuf<cplx> G; int lit[3];
        symbol_gv2d_literal(p.get(), box, G, lit);
        const int origin[3] = { 0, 0, 0 };
        plan_finish_from_literal(p.get(), G, lit, true, origin);
        p->even_dev = 0.0;                 // a function of kx^2 + ky^2 (plan_require_even_kernel)
        *out = p.release();
    });
}

int lsfc_plan_create_trap2d(lsfc_plan** out, int64_t n, int64_t m, double x0, double y0, double h, double omega,
                            double d0_re, double d0_im, const double* nu, unsigned flags, int device) {
    return guarded([&] {
        LSFC_REQUIRE(out, "NULL argument"); *out = nullptr;
        LSFC_REQUIRE(n % 2 == 1 && m % 2 == 1, "so far only works for n odd (src/FastConvolution.jl:455)");
        std::unique_ptr<lsfc_plan> p(new lsfc_plan());
        plan_common_init(p.get(), 2, n, m, 1, nu, omega, LSFC_QUAD_TRAPEZOIDAL, flags, device);
        DevBuf<cplx> G;
        symbol_trap2d_literal(p.get(), x0, y0, h, make_double2(d0_re, d0_im), G);
        const int lit[3] = { 2 * (int)n - 1, 2 * (int)m - 1, 1 };
        const int origin[3] = { (int)n - 1, (int)m - 1, 0 };
        plan_finish_from_literal(p.get(), G, lit, false, origin);
        // samples of a function of the distance to the centre of the extended grid (src/FastConvolution.jl:433-434): even where
        // the caller's grid is centred at the origin; any other grid is measured on first use (plan_require_even_kernel)
        if (fabs(x0 + (n - 1) / 2.0 * h) + fabs(y0 + (m - 1) / 2.0 * h) <= 1e-12 * fabs(h)) p->even_dev = 0.0;
        *out = p.release();
    });
}

int lsfc_plan_destroy(lsfc_plan* plan) {
    return guarded([&] {
        if (!plan) return;
        if (plan->multi) multi_synchronize(plan);
        else { (void)hipSetDevice(plan->device); (void)hipStreamSynchronize(plan->stream); }
        delete plan;
    });
}

int64_t lsfc_plan_size(const lsfc_plan* plan) { return plan ? plan->N : -1; }

int lsfc_plan_dims(const lsfc_plan* plan, int64_t dims[3], int64_t pads[3]) {
    return guarded([&] {
        LSFC_REQUIRE(plan, "NULL plan");
        for (int d = 0; d < 3; ++d) { if (dims) dims[d] = plan->dims[d]; if (pads) pads[d] = plan->pads[d]; }
    });
}

const char* lsfc_plan_pipeline(const lsfc_plan* plan) {
    if (!plan) return "";
    switch (plan->pipeline) {
    case lsfc_plan::PRUNED: return "pruned-hip";
    case lsfc_plan::ROCFFT_REDUCED: return "rocfft-reduced";
    default: return "rocfft-literal";
    }
}

// (kernel0 does not depend on nu: lsfc_plan_set_nu keeps it)
int lsfc_plan_set_nu(lsfc_plan* plan, const double* nu, int memspace) {
    return guarded([&] {
        LSFC_REQUIRE(plan && nu, "NULL argument");
        if (plan->multi) {
            LSFC_REQUIRE(memspace == LSFC_MEM_HOST, "a multi-device plan takes nu from the host");
            int64_t off = 0;
            for (auto& sp : plan->multi->sub) {
                LSFC_HIP(hipSetDevice(sp->device));
                LSFC_HIP(hipMemcpy(sp->nu.p, nu + off, sp->N * sizeof(double), hipMemcpyHostToDevice));
                off += sp->N;
            }
            return;
        }
        LSFC_HIP(hipSetDevice(plan->device));
        LSFC_HIP(hipMemcpyAsync(plan->nu.p, nu, plan->N * sizeof(double),
                                memspace == LSFC_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, plan->stream));
        LSFC_HIP(hipStreamSynchronize(plan->stream));
        plan->nu_im.release();           // back on the real path (the stream has drained: no pass still reads the plane)
    });
}
// N (re, im) pairs -> the planes nu and nu_im; every pass that multiplies by nu takes both from here on (apply.hip: slab_nu)
int lsfc_plan_set_nu_complex(lsfc_plan* plan, const double* nu, int memspace) {
    return guarded([&] {
        LSFC_REQUIRE(plan && nu, "NULL argument");
        LSFC_REQUIRE(!plan->multi, "complex nu is not available on a multi-device plan");
        LSFC_REQUIRE(!plan->dist, "complex nu is not available on a distributed (or simulated-rank) plan");
        LSFC_REQUIRE(memspace == LSFC_MEM_HOST || memspace == LSFC_MEM_DEVICE, "unknown memspace %d", memspace);
        LSFC_HIP(hipSetDevice(plan->device));
        const cplx* pairs = (const cplx*)nu;
        DevBuf<cplx> staged;
        if (memspace == LSFC_MEM_HOST) {
            staged.alloc((size_t)plan->N);
            LSFC_HIP(hipMemcpyAsync(staged.p, nu, (size_t)plan->N * sizeof(cplx), hipMemcpyHostToDevice, plan->stream));
            pairs = staged.p;
        }
        // both planes are made next to the plan's and swapped in together once they are complete: after an error the plan has
        // the nu it had
        DevBuf<double> re, im; re.alloc((size_t)plan->N); im.alloc((size_t)plan->N);
        pw_split_planes(pairs, re.p, im.p, plan->N, plan->stream);
        LSFC_HIP(hipStreamSynchronize(plan->stream));
        plan->nu = std::move(re);
        plan->nu_im = std::move(im);
    });
}
int lsfc_plan_nu_is_complex(const lsfc_plan* plan, int* is_complex) {
    return guarded([&] { LSFC_REQUIRE(plan && is_complex, "NULL argument"); *is_complex = plan->nu_im.p != nullptr; });
}

int lsfc_plan_get_symbol(const lsfc_plan* plan, double* out, int64_t capacity_complex, int64_t* count) {
    return guarded([&] {
        LSFC_REQUIRE(plan && count, "NULL argument");
        LSFC_REQUIRE(!plan->multi, "not available on a multi-device plan");
        *count = (int64_t)plan->sym.n;
        if (out) {
            LSFC_REQUIRE(capacity_complex >= (int64_t)plan->sym.n, "buffer too small");
            LSFC_HIP(hipMemcpy(out, plan->sym.p, plan->sym.bytes(), hipMemcpyDeviceToHost));
        }
    });
}

int lsfc_plan_set_stream(lsfc_plan* plan, void* hip_stream) {
    return guarded([&] {
        LSFC_REQUIRE(plan, "NULL plan");
        LSFC_REQUIRE(!plan->multi, "a multi-device plan runs on the streams of its ranks");
        plan->stream = (hipStream_t)hip_stream;
    });
}
int lsfc_plan_synchronize(lsfc_plan* plan) {
    return guarded([&] {
        LSFC_REQUIRE(plan, "NULL plan");
        if (plan->multi) { multi_synchronize(plan); return; }
        LSFC_HIP(hipSetDevice(plan->device)); LSFC_HIP(hipStreamSynchronize(plan->stream));
    });
}

int lsfc_plan_set_tuning(lsfc_plan* plan, const char* key, int value) {
    return guarded([&] {
        LSFC_REQUIRE(plan && key, "NULL argument");
        if (plan->multi) { for (auto& sp : plan->multi->sub) { const int rc = lsfc_plan_set_tuning(sp.get(), key, value); if (rc != LSFC_OK) fail(rc, "%s", lsfc_last_error()); } return; }
        for (const TuningKnob& k : TUNING_KNOBS) {
            if (!k.settable || strcmp(k.key, key) != 0) continue;
            if (k.flag) plan->tuning.*k.flag = value != 0;
            else plan->tuning.*k.value = value;
            return;
        }
        fail(LSFC_EINVAL, "unknown tuning key '%s'", key);
    });
}

int lsfc_device_count(int* count) {
    return guarded([&] { LSFC_REQUIRE(count, "NULL argument"); int c = 0; hipError_t e = hipGetDeviceCount(&c); *count = (e == hipSuccess) ? c : 0; });
}
int lsfc_malloc(void** dptr, size_t bytes, int device) {
    return guarded([&] { LSFC_REQUIRE(dptr, "NULL argument"); select_device(device, "lsfc operator", true); LSFC_HIP(hipMalloc(dptr, bytes)); });
}
int lsfc_free(void* dptr) { return guarded([&] { if (dptr) LSFC_HIP(hipFree(dptr)); }); }
int lsfc_memcpy_h2d(void* dst, const void* src, size_t bytes) { return guarded([&] { LSFC_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice)); }); }
int lsfc_memcpy_d2h(void* dst, const void* src, size_t bytes) { return guarded([&] { LSFC_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); }); }
int lsfc_host_register(void* ptr, size_t bytes) {
    return guarded([&] { LSFC_REQUIRE(ptr && bytes, "NULL argument"); LSFC_HIP(hipHostRegister(ptr, bytes, hipHostRegisterDefault)); });
}
int lsfc_host_unregister(void* ptr) { return guarded([&] { LSFC_REQUIRE(ptr, "NULL argument"); LSFC_HIP(hipHostUnregister(ptr)); }); }
int lsfc_host_alloc(void** ptr, size_t bytes) {
    return guarded([&] { LSFC_REQUIRE(ptr && bytes, "NULL argument"); *ptr = nullptr; LSFC_HIP(hipHostMalloc(ptr, bytes, hipHostMallocDefault)); });
}
int lsfc_host_free(void* ptr) { return guarded([&] { if (ptr) LSFC_HIP(hipHostFree(ptr)); }); }

} // extern "C"
