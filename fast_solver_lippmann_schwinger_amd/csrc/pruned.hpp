// Host-side interface of the hand-written pruned axis passes (fft_kernels.hip).
#pragma once
#include "common.hpp"

namespace lsfc {

// Several right-hand sides through one pipeline (lsfc_apply_batch, the batched GMRES): the x passes take the user
// vectors of all of them (arbitrary pointers), the work arrays hold the batch back to back, and the fused pass loads
// every symbol tile ONCE for the whole batch.
static constexpr int LSFC_MAX_BATCH = 8;
struct VecBatch {
    const cplx* x[LSFC_MAX_BATCH];
    cplx* y[LSFC_MAX_BATCH];
};

struct PrunedTuning {
    bool split_x = true;   // contiguous (x) passes: exchange re/im separately (half the LDS, twice the barriers)
    bool split_s = true;   // strided y passes
    int split_z = -1;      // fused z pass: 1 split, 0 whole complex, -1 auto (by line length)
    int sym_prefetch = -1; // z pass: load the symbol before the forward transform; -1 auto
    int pad1 = -1, pad2 = -1;        // row padding (elements, multiples of 8) of the A1 rows / A2 tile rows, read at plan creation
    int tw_lds = 1;                 // fused pass (full-tile form): stage twiddles from an LDS-resident table instead of product
                                    // trees (-2..3 % on the pass, exact twiddles; profiles/r01_experiment_lds_twiddle_table.log)
    int z_half = -1;                // L = 1024 z pass: half-tile 4-wave workgroups (0 off, 1: full+prefetch, 2: split+prefetch, 3: split 3 WG/CU, 4: full; -1 auto)
    int z_persist = -1;             // fused pass with a z-even symbol in the 3D layout: persistent software-pipelined kernel -- 1 whole-complex
                                    // exchanges, 2 split exchanges, 3 (auto) / 4 the same with the symbol loaded after the first forward
                                    // stage; 0 the one-tile-per-workgroup kernels
    int xlane = -1;                 // fused pass, lines with two consecutive stages of equal radix (8.8: 512, 1024, 1536 points; 4.4: 128, 192,
                                    // 320, 384, 640, 1280): the exchange between them through the lanes of the wavefront instead of LDS
                                    // (1 / -1 auto: on; 0: LDS)
    int ytile_g = 0, ytile_z = 0;   // y passes: block-order tile (x'-groups x z planes); 0 = auto
    int batch_fuse = -1;            // several right-hand sides: 1 one fused pass per group, 0 member by member, -1 auto (fused while
                                    // the padded grid has <= 2^24 points, where launches and not bytes bound the apply:
                                    // profiles/r02_batch_apply.jsonl -- 2.3x per right-hand side at 48^3, -5 % at 256^3)
};
// Every knob once: its lsfc_plan_set_tuning key, the environment variable that sets its default at plan creation
// (pruned_default_tuning), its field -- a flag or an integer --, and whether it can still be set on a finished plan.
//   environment, flag:    unset or empty keeps the default; a first character 1, y or t is true, anything else false
//   environment, integer: atoi whenever the variable is set
//   set_tuning:           value != 0 for a flag, the value itself for an integer
struct TuningKnob { const char* key; const char* env; bool PrunedTuning::* flag; int PrunedTuning::* value; bool settable; };
inline constexpr TuningKnob TUNING_KNOBS[] = {
    {"split_x", "LSFC_SPLIT_X", &PrunedTuning::split_x, nullptr, true},
    {"split_s", "LSFC_SPLIT_S", &PrunedTuning::split_s, nullptr, true},
    {"split_z", "LSFC_SPLIT_Z", nullptr, &PrunedTuning::split_z, true},
    {"pad1", "LSFC_PAD1", nullptr, &PrunedTuning::pad1, false},          // (the work arrays are laid out at plan creation)
    {"pad2", "LSFC_PAD2", nullptr, &PrunedTuning::pad2, false},
    {"z_half", "LSFC_Z_HALF", nullptr, &PrunedTuning::z_half, true},
    {"tw_lds", "LSFC_TW_LDS", nullptr, &PrunedTuning::tw_lds, true},
    {"sym_prefetch", "LSFC_SYM_PREFETCH", nullptr, &PrunedTuning::sym_prefetch, true},
    {"ytile_g", "LSFC_YTILE_G", nullptr, &PrunedTuning::ytile_g, true},
    {"ytile_z", "LSFC_YTILE_Z", nullptr, &PrunedTuning::ytile_z, true},
    {"batch_fuse", "LSFC_BATCH_FUSE", nullptr, &PrunedTuning::batch_fuse, true},
    {"z_persist", "LSFC_Z_PERSIST", nullptr, &PrunedTuning::z_persist, true},
    {"xlane", "LSFC_XLANE", nullptr, &PrunedTuning::xlane, true},
};

bool pruned_length_supported(int64_t L);
// load EVERY code object of the library on `device` (the current device) once, ahead of the first transfer or pass (fft_kernels.hip)
void pruned_warmup(int device);
// smallest supported line length L >= max(2n, 32): L = 2^k, 3 * 2^k or 5 * 2^k (0: none up to 2048)
int pruned_best_length(int64_t n);
// n (x passes), m (y passes), nin (fused pass): the actual grid size along the transformed axis, <= L/2; entries beyond
// it are treated as zero on the way in and not written on the way back.
// W = chunk width of the x'-storage axis in the xfwd output / xinv input: out[s / W][line][s % W] (W = L on one GPU;
// W = L / nranks packs the slab transpose for free).
// freq_of_storage[s] = frequency index held at storage index s after the forward pass of length L
void pruned_perm(int L, int* freq_of_storage);
PrunedTuning pruned_default_tuning();

// Re nu and Im nu (null: nu is real) of the plan, or of a pass: both null where the pass does not multiply
struct NuPlanes { const double* re; const double* im; };

// What a pass takes, by name: plain aggregates (no defaults -- a site that fills one names every field).
// nrhs / vb / *batch: right-hand sides per launch (<= LSFC_MAX_BATCH), their vectors, and the distance between the
// batch members in the work arrays.
// The x passes.  xfwd: work = transform of (nu ? nu : 1) .* x, with conj of conj(nu .* x) for a real nu and of nu .* conj(x) for a
// complex one.  xinv: y = alpha*x + beta * (nu ? nu : 1) .* (conj ? conj(v) : v), v the cropped inverse transform of work; with
// conj the factor of a complex nu is conj(nu) (the conjugation is outermost: plan.hpp, ConvOp).  nu like x is indexed as y is.
struct XPass {
    int L;                  // line length
    VecBatch vb; int nrhs;
    cplx* work;             // [chunk][line][Wp]: written by xfwd, read by xinv
    int64_t wbatch;
    const cplx* tw;
    int64_t nlines;
    int W, Wp, n;
    int64_t bstride;        // distance between chunks of the storage axis (0: dense, Wp * nlines)
    NuPlanes nu;
    bool conj;
    double alpha, beta;     // (xinv only)
};
// The y passes, yfwd a1 -> a2 and yinv a2 -> a1.  p1: row pitch of A1 (>= Lx), p2: pitch of one storage-y row of an A2 tile
// (>= 8*l); both multiples of 8 elements
struct YPass {
    int L;
    cplx* a1; cplx* a2;
    const cplx* tw;
    int Lx, m, l, p1, p2;
    int nrhs;
    int64_t batch1, batch2;
};
// full stage-twiddle table of the factorisation used for length L (host side; tw[j] = exp(-2 pi i j / L))
int pruned_twfull_len(int L);
void pruned_twfull(int L, const cplx* tw, cplx* out);
// Geometry of one fused pass (forward transform along the line, multiply by the symbol, inverse transform, in place).
// Lines come in tiles of 8 consecutive x' storage indices; `nouter` lines of the other transformed axis share a tile.
// Line (tile g, row o, xi in 0..7): element j at data[g*dTile + o*dOuter + xi + dLine*j], the symbol value of storage
// index j at sym[g*sTile + so*sOuter + xi + sLine*j]; block b of a tile takes (o, so) = ytab[b], or (b, b) without a table.
struct FusedGeom {
    int Lx;                 // x' storage indices covered (a multiple of 8): Lx / 8 tiles
    int nouter;             // lines per (tile, xi): Ly in 3D, 1 in 2D
    int64_t dTile, dOuter, dLine;   // strides of `data` per tile, per outer line, per element of a line
    int64_t sTile, sOuter, sLine;   // the same for the symbol
    const int2* ytab;       // block order -> (data row, symbol row); NULL: identity
    const int* zm;          // even symbol: partner storage index of every upper-half slot; NULL: full symbol lines
    int nin;                // valid entries per line (<= L/2)
};
// What a pass launches: the kernel family and the template flags of the instantiation.  Every pass has a pure host function
// (no launch, no device access) from the inputs its dispatcher has to this description; the launchers switch on the description
// and on nothing else, and lsfc_plan_describe_passes prints it, so that a test can see which kernel a tuning request selects.
enum class PassFamily { XFWD, XINV, YFWD, YINV, ZFUSED, ZFUSED_HALF, ZFUSED_PERSIST, ZFUSED_PERSIST_HALF };
// xfwd, xinv, yfwd, yinv, zfused, zfused_half, zfused_persist, zfused_persist_half
const char* pass_family_name(PassFamily);
struct PassForm {
    PassFamily family = PassFamily::XFWD;
    int L = 0;
    bool split = false;            // SPLIT: re/im-split LDS exchanges
    bool forced_split = false;     // y passes: split because whole-complex exchanges exceed the LDS, whatever split_s says
    bool prefetch = false;         // PREFETCH: symbol loaded before the forward transform (one-tile fused kernels)
    bool ze = false;               // ZE: z-even half symbol lines (mirror slots)
    bool full = false;             // FULL: the grid fills the line (n == L/2), end-of-line predicates compiled away
    bool twl = false;              // TWL: stage twiddles from the LDS-resident table
    bool batch = false;            // BATCH: one launch for all right-hand sides, one symbol load per tile
    bool late_sym = false;         // LATE_SYM: persistent forms, symbol loaded after the first forward stage
    bool tickets = false;          // TICKETS: tiles handed out by per-XCD ticket counters
    int xl = 0;                    // XL: lane exchanges between stages of equal radix (persistent forms: 0, 1, 3, 5; one-tile kernels: 0 / 1,
                                   // not a choice there but the kernels' own constexpr, fft_kernels.hip xl_one_tile)
    int lines = 0;                 // LINES: lines per workgroup (y and fused passes)
    int wpe = 1;                   // WPE: workgroups per CU the kernel is bounded for (its __launch_bounds__)
    int tg = 0, tz = 0;            // y passes: resolved block-order tile (x'-groups x z planes)
    bool per_member = false;       // a batch that runs through this form member by member (one launch per right-hand side)
};
// The fused pass.  twl: full stage-twiddle table of the line, or NULL; dBatch: distance between the batch members in `data`
struct FusedPass {
    int L;
    cplx* data;
    const cplx* sym;
    const cplx* tw;
    const cplx* twl;
    FusedGeom g;
    int nrhs;
    int64_t dBatch;
};
PassForm pruned_xfwd_form(const PrunedTuning&, const XPass&);
PassForm pruned_xinv_form(const PrunedTuning&, const XPass&);
PassForm pruned_yfwd_form(const PrunedTuning&, const YPass&);
PassForm pruned_yinv_form(const PrunedTuning&, const YPass&);
PassForm pruned_zfused_form(const PrunedTuning&, const FusedPass&);
// "family L=.. SPLIT=.. ..." (one line, no newline) into buf; returns the length written
int pass_form_print(const PassForm&, char* buf, size_t cap);

void pruned_xfwd(const PrunedTuning&, const XPass&, hipStream_t);
void pruned_xinv(const PrunedTuning&, const XPass&, hipStream_t);
void pruned_yfwd(const PrunedTuning&, const YPass&, hipStream_t);
void pruned_yinv(const PrunedTuning&, const YPass&, hipStream_t);
void pruned_zfused(const PrunedTuning&, const FusedPass&, hipStream_t);

// What one compilation of fft_kernels.hip exports (pruned_family_f2, _f3, _f5): the launchers and the host tables of its lines.
// pruned.hip routes every call above through the table of the line's family.
struct PrunedFamily {
    void (*xfwd)(const PrunedTuning&, const XPass&, hipStream_t);
    void (*xinv)(const PrunedTuning&, const XPass&, hipStream_t);
    void (*yfwd)(const PrunedTuning&, const YPass&, hipStream_t);
    void (*yinv)(const PrunedTuning&, const YPass&, hipStream_t);
    void (*zfused)(const PrunedTuning&, const FusedPass&, hipStream_t);
    PassForm (*xform)(PassFamily, const PrunedTuning&, const XPass&);
    PassForm (*yform)(PassFamily, const PrunedTuning&, const YPass&);
    PassForm (*zfused_form)(const PrunedTuning&, const FusedPass&);
    void (*perm)(int L, int* freq_of_storage);
    int (*twfull_len)(int L);
    void (*twfull)(int L, const cplx* tw, cplx* out);
    void (*warmup)();
};

} // namespace lsfc
